"""utils/visibility.py's contract restated with Python floats (IEEE doubles: one rounding per operation), one (point, view) pair at a
time: the march of a ray through the occupancy grid, and the packing of the bits into words."""
import math

import numpy as np


def ray_visible(p, c, occ, origin, h, dims, i0, skip, max_blocked):
    """True unless the ray from p (start voxel i0) to the centre c is blocked."""
    step, tmax, td = [0, 0, 0], [math.inf] * 3, [0.0] * 3
    for a in range(3):
        D = c[a] - p[a]
        if D > 0.0:
            step[a], tmax[a], td[a] = 1, ((origin[a] + (i0[a] + 1) * h) - p[a]) / D, h / D
        elif D < 0.0:
            step[a], tmax[a], td[a] = -1, ((origin[a] + i0[a] * h) - p[a]) / D, h / (-D)
    i, blocked = list(i0), 0
    for _ in range(dims[0] + dims[1] + dims[2]):
        a = 0
        if tmax[1] < tmax[a]:
            a = 1
        if tmax[2] < tmax[a]:
            a = 2
        if not tmax[a] < 1.0:
            return True
        i[a] += step[a]
        if i[a] < 0 or i[a] >= dims[a]:
            return True
        tmax[a] = tmax[a] + td[a]
        if max(abs(i[0] - i0[0]), abs(i[1] - i0[1]), abs(i[2] - i0[2])) > skip and occ[i[2], i[1], i[0]] != 0:
            blocked += 1
            if blocked > max_blocked:
                return False
    raise AssertionError("the cap of nx + ny + nz steps was reached: the contract says it cannot be")


def visible_loop(points, centres, occ, origin, h, skip=1, max_blocked=0):
    """bool [N, V]: view k is not blocked for point i."""
    pts, C = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(centres, np.float64).reshape(-1, 3)
    nz, ny, nx = occ.shape
    dims = (nx, ny, nz)
    origin, h = [float(o) for o in origin], float(h)
    out = np.ones((pts.shape[0], C.shape[0]), bool)
    for n in range(pts.shape[0]):
        p = [float(v) for v in pts[n]]
        t = [(p[a] - origin[a]) / h for a in range(3)]
        if not all(t[a] >= 0.0 and t[a] < dims[a] for a in range(3)):
            continue                                             # (a NaN too: unoccluded)
        i0 = [int(math.floor(t[a])) for a in range(3)]
        for k in range(C.shape[0]):
            out[n, k] = ray_visible(p, [float(v) for v in C[k]], occ, origin, h, dims, i0, skip, max_blocked)
    return out


def words_of(visible):
    """int32 [N, ceil(V/32)] of bool [N, V], bit by bit."""
    N, V = visible.shape
    words = np.zeros((N, (V + 31) // 32), np.int64)
    for n in range(N):
        for k in range(V):
            if visible[n, k]:
                words[n, k // 32] |= 1 << (k % 32)
    return np.ascontiguousarray(words.astype(np.uint32).view(np.int32))
