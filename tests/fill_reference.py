"""utils/field_fill.py's contract restated with Python floats (IEEE doubles: one rounding per operation) and a plain triple loop over
the nodes, independent of that module."""
import math

import numpy as np

OUT, FREE, FIXED = 0, 1, 2
STEPS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))     # -x, +x, -y, +y, -z, +z


def classify(dirs, conf, fixed_conf, allowed=None):
    nz, ny, nx = conf.shape
    kind = np.zeros((nz, ny, nx), np.uint8)
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                if float(conf[iz, iy, ix]) >= fixed_conf and all(math.isfinite(float(c)) for c in dirs[iz, iy, ix]):
                    kind[iz, iy, ix] = FIXED
                elif allowed is None or bool(allowed[iz, iy, ix]):
                    kind[iz, iy, ix] = FREE
    return kind


def seed(dirs, kind):
    nz, ny, nx = kind.shape
    T = np.zeros((6, nz, ny, nx), np.float64)
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                if kind[iz, iy, ix] == FIXED:
                    d = [float(c) for c in dirs[iz, iy, ix]]
                    T[:, iz, iy, ix] = [d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]]
    return T


def sweep(T, kind):
    nz, ny, nx = kind.shape
    new = T.copy()
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                if kind[iz, iy, ix] != FREE:
                    continue
                for j in range(6):
                    s, c = 0.0, 0
                    for dx, dy, dz in STEPS:
                        x, y, z = ix + dx, iy + dy, iz + dz
                        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and kind[z, y, x] != OUT:
                            s = s + float(T[j, z, y, x])
                            c = c + 1
                        else:
                            s = s + 0.0
                    new[j, iz, iy, ix] = s / float(c) if c > 0 else float(T[j, iz, iy, ix])
    return new


def fill(T, kind, sweeps):
    """(the iterate after `sweeps` sweeps, the one before it); sweeps = 0: T twice."""
    res, prev = T.copy(), T.copy()
    for _ in range(sweeps):
        res, prev = sweep(res, kind), res
    return res, prev
