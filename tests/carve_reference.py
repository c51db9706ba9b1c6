"""The contract of utils/carve.py restated as plain Python loops over points, views and voxels: Python floats (float64, one rounding
per operation), math.floor, no numpy arithmetic.  Slow; meant for the small cases of tests/test_carve_cpu.py."""
import math

import numpy as np


def vote(view, mask, x, y, z):
    """(seen, hit, py, px) of one point in one view."""
    R = [[float(view.R[i][j]) for j in range(3)] for i in range(3)]
    t = [float(view.t[i]) for i in range(3)]
    x, y, z = float(x), float(y), float(z)
    xc = ((R[0][0] * x + R[0][1] * y) + R[0][2] * z) + t[0]
    yc = ((R[1][0] * x + R[1][1] * y) + R[1][2] * z) + t[1]
    zc = ((R[2][0] * x + R[2][1] * y) + R[2][2] * z) + t[2]
    if math.isnan(zc) or not zc > 0.0:
        return False, False, 0, 0
    qx, qy = xc / zc, yc / zc                      # (zc > 0: Python divides as IEEE does, inf and NaN included)
    u = float(view.fx) * qx + float(view.cx)
    v = float(view.fy) * qy + float(view.cy)
    if not (0.0 <= u < view.W and 0.0 <= v < view.H):
        return False, False, 0, 0
    px, py = math.floor(u), math.floor(v)
    return True, int(mask[py][px]) != 0, py, px


def mask_votes(points, views, masks, images=None):
    n = len(points)
    seen, hits = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rgb = np.zeros((n, 3), np.int32)
    for i in range(n):
        for k, view in enumerate(views):
            s, hit, py, px = vote(view, masks[k], points[i][0], points[i][1], points[i][2])
            if s:
                seen[i] += 1
            if hit:
                hits[i] += 1
                if images is not None:
                    for c in range(3):
                        rgb[i][c] += int(images[k][py][px][c])
    return (seen, hits, rgb) if images is not None else (seen, hits)


def kept(seen, hits, min_views, min_percent):
    return int(seen) >= min_views and 100 * int(hits) >= min_percent * int(seen)


def carve_grid(origin, h, dims, views, masks, min_views, min_percent):
    nx, ny, nz = dims
    occ = np.zeros((nz, ny, nx), np.uint8)
    o, h = [float(v) for v in origin], float(h)
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                p = [(o[0] + (ix + 0.5) * h, o[1] + (iy + 0.5) * h, o[2] + (iz + 0.5) * h)]
                seen, hits = mask_votes(p, views, masks)
                occ[iz][iy][ix] = 1 if kept(seen[0], hits[0], min_views, min_percent) else 0
    return occ


def shell(occ):
    nz, ny, nx = occ.shape
    out = np.zeros_like(occ)

    def filled(z, y, x):
        return 0 <= z < nz and 0 <= y < ny and 0 <= x < nx and occ[z][y][x] != 0
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                if occ[z][y][x] and not all(filled(z + dz, y + dy, x + dx) for dz, dy, dx in
                                            ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))):
                    out[z][y][x] = 1
    return out


def dilate(mask, r):
    H, W = mask.shape
    out = np.zeros_like(mask)
    for y in range(H):
        for x in range(W):
            out[y][x] = max(int(mask[yy][xx]) for yy in range(max(0, y - r), min(H, y + r + 1))
                            for xx in range(max(0, x - r), min(W, x + r + 1)))
    return out
