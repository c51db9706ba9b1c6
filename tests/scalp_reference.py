"""The contract of utils/scalp.py restated as plain Python loops over faces, pixels, samples and views: Python floats (float64, one
rounding per operation), math.floor / math.ceil, no numpy arithmetic.  Slow; meant for the small cases of tests/test_scalp_cpu.py."""
import math

import numpy as np

INF = float("inf")


def _camera(view, x, y, z):
    R = [[float(view.R[i][j]) for j in range(3)] for i in range(3)]
    t = [float(view.t[i]) for i in range(3)]
    x, y, z = float(x), float(y), float(z)
    xc = ((R[0][0] * x + R[0][1] * y) + R[0][2] * z) + t[0]
    yc = ((R[1][0] * x + R[1][1] * y) + R[1][2] * z) + t[1]
    zc = ((R[2][0] * x + R[2][1] * y) + R[2][2] * z) + t[2]
    return xc, yc, zc


def _image(view, xc, yc, zc):
    """(u, v) of a point with zc > 0 (Python divides as IEEE does there, inf and NaN included)."""
    return float(view.fx) * (xc / zc) + float(view.cx), float(view.fy) * (yc / zc) + float(view.cy)


def depth_map(view, verts, faces):
    """(Z, dropped): Z a list of H rows of W floats."""
    W, H = int(view.W), int(view.H)
    Z = [[INF] * W for _ in range(H)]
    dropped = 0
    for face in faces:
        u, v, iz = [], [], []
        for i in face:
            xc, yc, zc = _camera(view, *verts[int(i)])
            if not zc > 0.0:                                     # (a NaN included)
                break
            ui, vi = _image(view, xc, yc, zc)
            if not (math.isfinite(ui) and math.isfinite(vi)):
                break
            u.append(ui)
            v.append(vi)
            iz.append(1.0 / zc)
        if len(u) < 3:
            dropped += 1
            continue
        x0 = max(0.0, math.ceil(min(u) - 0.5))
        x1 = min(W - 1.0, math.floor(max(u) - 0.5))
        y0 = max(0.0, math.ceil(min(v) - 0.5))
        y1 = min(H - 1.0, math.floor(max(v) - 0.5))
        for py in range(int(y0), int(y1) + 1):
            for px in range(int(x0), int(x1) + 1):
                cx, cy = px + 0.5, py + 0.5
                E0 = (u[2] - u[1]) * (cy - v[1]) - (v[2] - v[1]) * (cx - u[1])
                E1 = (u[0] - u[2]) * (cy - v[2]) - (v[0] - v[2]) * (cx - u[2])
                E2 = (u[1] - u[0]) * (cy - v[0]) - (v[1] - v[0]) * (cx - u[0])
                S = (E0 + E1) + E2
                if not (S != 0.0 and ((E0 >= 0.0 and E1 >= 0.0 and E2 >= 0.0) or (E0 <= 0.0 and E1 <= 0.0 and E2 <= 0.0))):
                    continue
                q = (E0 * iz[0] + E1 * iz[1]) + E2 * iz[2]
                if q == 0.0 or math.isnan(q) or math.isnan(S):  # (S/0 is an infinity or a NaN: never stored)
                    continue
                z = S / q
                if math.isfinite(z) and z > 0.0 and z < Z[py][px]:
                    Z[py][px] = z
    return Z, dropped


def depth_maps(verts, faces, views):
    maps, dropped = [], 0
    for view in views:
        Z, d = depth_map(view, verts, faces)
        maps.append(np.array(Z, np.float64).reshape(int(view.H), int(view.W)))
        dropped += d
    return maps, dropped


def scalp_votes(points, normals, views, masks, depth, min_cos, depth_tol):
    n = len(points)
    vis, hits = np.zeros(n, np.int32), np.zeros(n, np.int32)
    min_cos, depth_tol = float(min_cos), float(depth_tol)
    for i in range(n):
        n0, n1, n2 = (float(a) for a in normals[i])
        for k, view in enumerate(views):
            xc, yc, zc = _camera(view, *points[i])
            if not zc > 0.0:
                continue
            u, v = _image(view, xc, yc, zc)
            if not (0.0 <= u < view.W and 0.0 <= v < view.H):
                continue
            px, py = math.floor(u), math.floor(v)
            R = view.R
            nc = [(float(R[r][0]) * n0 + float(R[r][1]) * n1) + float(R[r][2]) * n2 for r in range(3)]
            d = -((nc[0] * xc + nc[1] * yc) + nc[2] * zc)
            nn = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]
            pp = (xc * xc + yc * yc) + zc * zc
            if not (d > 0.0 and d * d >= (min_cos * min_cos) * (nn * pp)):
                continue
            if not zc <= float(depth[k][py][px]) + depth_tol:
                continue
            vis[i] += 1
            if int(masks[k][py][px]) != 0:
                hits[i] += 1
    return vis, hits
