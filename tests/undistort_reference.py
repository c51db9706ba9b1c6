"""The undistortion contract restated pixel by pixel in plain Python floats (float64, one rounding per operation), independent of
hair-gs_amd/utils/undistort.py: the model table, img_from_cam, and the warp with its validity rule and two output modes.  Meant for
the small sizes of tests/test_undistort_cpu.py."""
import math

import numpy as np


def distortion(model, params, u, v):
    """(fx, fy, cx, cy, du, dv) of one normalised point."""
    p = [float(x) for x in params]
    if model in ("SIMPLE_RADIAL", "RADIAL"):
        fx = fy = p[0]
        cx, cy = p[1], p[2]
    else:
        fx, fy, cx, cy = p[0], p[1], p[2], p[3]
    uu = u * u
    vv = v * v
    r2 = uu + vv
    if model == "SIMPLE_RADIAL":
        rad = p[3] * r2
    elif model == "RADIAL":
        rad = p[3] * r2 + p[4] * (r2 * r2)
    elif model == "OPENCV":
        rad = p[4] * r2 + p[5] * (r2 * r2)
    elif model == "FULL_OPENCV":
        r4 = r2 * r2
        r6 = r4 * r2
        num = ((1.0 + p[4] * r2) + p[5] * r4) + p[8] * r6
        den = ((1.0 + p[9] * r2) + p[10] * r4) + p[11] * r6
        rad = num / den - 1.0
    else:
        raise ValueError(model)
    du = u * rad
    dv = v * rad
    if model in ("OPENCV", "FULL_OPENCV"):
        p1, p2 = p[6], p[7]
        uv = u * v
        du = (du + (2.0 * p1) * uv) + p2 * (r2 + 2.0 * uu)
        dv = (dv + (2.0 * p2) * uv) + p1 * (r2 + 2.0 * vv)
    return fx, fy, cx, cy, du, dv


def img_from_cam(model, params, u, v):
    fx, fy, cx, cy, du, dv = distortion(model, params, u, v)
    return fx * (u + du) + cx, fy * (v + dv) + cy


def undistort(images, model, params, pinhole, out_size, mode):
    """images uint8 [N, H, W, C]; pinhole = (fx', fy', cx', cy') and out_size = (W', H') of the output camera;
    mode "bilinear" or "threshold" -> (out uint8 [N, H', W', C], valid bool [H', W'])."""
    N, H, W, C = images.shape
    fxd, fyd, cxd, cyd = (float(x) for x in pinhole)
    Wd, Hd = out_size
    out = np.zeros((N, Hd, Wd, C), np.uint8)
    valid = np.zeros((Hd, Wd), bool)
    for y in range(Hd):
        for x in range(Wd):
            u = ((x + 0.5) - cxd) / fxd
            v = ((y + 0.5) - cyd) / fyd
            X, Y = img_from_cam(model, params, u, v)
            sx = X - 0.5
            sy = Y - 0.5
            if not (0.0 <= sx <= W - 1 and 0.0 <= sy <= H - 1):
                continue
            valid[y, x] = True
            x0 = math.floor(sx)
            y0 = math.floor(sy)
            x1 = min(x0 + 1, W - 1)
            y1 = min(y0 + 1, H - 1)
            wx = sx - x0
            wy = sy - y0
            for n in range(N):
                for c in range(C):
                    p00, p01 = float(images[n, y0, x0, c]), float(images[n, y0, x1, c])
                    p10, p11 = float(images[n, y1, x0, c]), float(images[n, y1, x1, c])
                    value = (1.0 - wy) * ((1.0 - wx) * p00 + wx * p01) + wy * ((1.0 - wx) * p10 + wx * p11)
                    out[n, y, x, c] = math.floor(value + 0.5) if mode == "bilinear" else (255 if value >= 127.5 else 0)
    return out, valid
