"""The groom interpolation's contract (scene/groom.py, csrc/hgs_groom.hip) restated as a plain Python loop: one root, one guide, one
rank, one point and one coordinate at a time, on Python floats (IEEE float64, one rounding per operation).  Nothing here is shared
with the product code.  Every comparison against it is bit for bit (tests/test_groom_cpu.py, tests/test_groom_gpu.py)."""
import functools
import math

import numpy as np

INF = math.inf


def _f(x):
    return float(x)          # float32 / float64 -> Python float, exactly


def chords(gp):
    """[(cx, cy, cz, len)] per guide."""
    out = []
    for g in range(gp.shape[0]):
        cx, cy, cz = (_f(gp[g, -1, c]) - _f(gp[g, 0, c]) for c in range(3))
        out.append((cx, cy, cz, math.sqrt((cx * cx + cy * cy) + cz * cz)))
    return out


def candidates(gp, roots):
    """Per root, ALL its candidates [(d2, g)] with a finite d2, sorted by (d2, g): what a search with any k and max_d2 chooses from."""
    g0 = [[_f(gp[g, 0, c]) for c in range(3)] for g in range(gp.shape[0])]
    out = []
    for n in range(roots.shape[0]):
        rx, ry, rz = (_f(roots[n, c]) for c in range(3))
        cand = []
        for g, (gx, gy, gz) in enumerate(g0):
            dx, dy, dz = rx - gx, ry - gy, rz - gz
            d2 = (dx * dx + dy * dy) + dz * dz
            if math.isfinite(d2):
                cand.append((d2, g))
        cand.sort()
        out.append(cand)
    return out


def search(cands, ch, k, max_d2, cos_max):
    """(idx int32 [N, k], d2 float64 [N, k], w float64 [N, k], count int32 [N]) from candidates() and chords()."""
    N = len(cands)
    idx, d2o = np.full((N, k), -1, np.int32), np.full((N, k), np.inf, np.float64)
    wo, count = np.zeros((N, k), np.float64), np.zeros(N, np.int32)
    for n, cand in enumerate(cands):
        lst = [(d2, g) for d2, g in cand if not d2 > max_d2][:k]
        if not lst:
            continue
        d0, g0 = lst[0]
        c0 = ch[g0]
        kept = [(d0, g0, 1.0)]
        for d2, g in lst[1:]:
            if d0 == 0.0:
                break
            ci = ch[g]
            dot = (ci[0] * c0[0] + ci[1] * c0[1]) + ci[2] * c0[2]
            if ci[3] > 0.0 and c0[3] > 0.0 and dot >= cos_max * (ci[3] * c0[3]):
                kept.append((d2, g, d0 / d2))
        W = 0.0
        for _, _, w in kept:
            W = W + w
        for i, (d2, g, w) in enumerate(kept):
            idx[n, i], d2o[n, i], wo[n, i] = g, d2, w / W
        count[n] = len(kept)
    return idx, d2o, wo, count


def blend(gp, ga, roots, idx, w, count):
    """(points float32 [n_kept M, 3], attrs float32 [n_kept M, C], kept int64) of the roots with count > 0."""
    M, C = gp.shape[1], ga.shape[2]
    gpl, gal = gp.astype(np.float64).tolist(), ga.astype(np.float64).tolist()     # (float32 -> float64 is exact)
    pts, att, kept = [], [], []
    with np.errstate(all="ignore"):
        for n in range(roots.shape[0]):
            if count[n] == 0:
                continue
            kept.append(n)
            gs = [int(idx[n, i]) for i in range(count[n])]
            ws = [float(w[n, i]) for i in range(count[n])]
            for j in range(M):
                p = []
                for c in range(3):
                    acc = 0.0
                    for g, wt in zip(gs, ws):
                        acc = acc + wt * (gpl[g][j][c] - gpl[g][0][c])
                    p.append(np.float32(float(roots[n, c]) + acc))
                pts.append(p)
                a = []
                for q in range(C):
                    acc = 0.0
                    for g, wt in zip(gs, ws):
                        acc = acc + wt * gal[g][j][q]
                    a.append(np.float32(acc))
                att.append(a)
    return (np.array(pts, np.float32).reshape(-1, 3), np.array(att, np.float32).reshape(-1, C), np.array(kept, np.int64))


def lengths(pts, M):
    """float64 polyline length of float32 strands of M points, segment by segment."""
    out = []
    for s in range(pts.shape[0] // M):
        L = 0.0
        for j in range(M - 1):
            dx, dy, dz = (float(pts[s * M + j + 1, c]) - float(pts[s * M + j, c]) for c in range(3))
            L = L + math.sqrt((dx * dx + dy * dy) + dz * dz)
        out.append(L)
    return np.array(out, np.float64)


# The candidates of the size grid's cases, computed once per K and shared by every test that needs them (CPU and GPU modules alike).
@functools.lru_cache(maxsize=None)
def grid_candidates(K):
    from tests import groom_cases as GC
    gp, _, roots = GC.grid_case(K)
    return candidates(gp, roots), chords(gp)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
