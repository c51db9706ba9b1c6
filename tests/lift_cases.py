"""Rigs, planes, the loop restatement and the comparison rule shared by tests/test_lift_cpu.py and tests/test_lift_gpu.py."""
import math
import os

import numpy as np

from tests import carve_cases as CC

STEP_DEG = 180.0 / 255.0           # one quantisation step of the orientation byte


# ---- the contract, restated with Python floats (IEEE doubles: one rounding per operation) ------------------------------
def moments_loop(points, views, masks, orients, confs, tab, prev=None, s2=0.0, min_conf=1):
    """utils/lift.py's moments, point by point and view by view: (M [N, 6], wsum [N], count [N])."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    N = pts.shape[0]
    M, wsum, count = np.zeros((N, 6), np.float64), np.zeros(N, np.float64), np.zeros(N, np.int32)
    T = [(float(tab[o, 0]), float(tab[o, 1])) for o in range(256)]
    for i in range(N):
        x, y, z = (float(c) for c in pts[i])
        p = None if prev is None else [float(c) for c in prev[i]]
        if p is not None and p[0] == 0.0 and p[1] == 0.0 and p[2] == 0.0:
            p = None
        m, ws, cnt = [0.0] * 6, 0.0, 0
        for k, v in enumerate(views):
            R = [[float(v.R[r, c]) for c in range(3)] for r in range(3)]
            t = [float(c) for c in v.t]
            xc = ((R[0][0] * x + R[0][1] * y) + R[0][2] * z) + t[0]
            yc = ((R[1][0] * x + R[1][1] * y) + R[1][2] * z) + t[1]
            zc = ((R[2][0] * x + R[2][1] * y) + R[2][2] * z) + t[2]
            if not zc > 0.0:                                     # (also a NaN, and keeps the division away from zero)
                continue
            u = v.fx * (xc / zc) + v.cx
            w_ = v.fy * (yc / zc) + v.cy
            if not (u >= 0.0 and u < v.W and w_ >= 0.0 and w_ < v.H):
                continue
            px, py = int(math.floor(u)), int(math.floor(w_))
            if masks[k][py, px] == 0 or int(confs[k][py, px]) < min_conf:
                continue
            lu, lv = T[int(orients[k][py, px])]
            a, b = lu / v.fx, lv / v.fy
            ncx, ncy, ncz = -(zc * b), zc * a, xc * b - yc * a
            n = [(R[0][j] * ncx + R[1][j] * ncy) + R[2][j] * ncz for j in range(3)]
            nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            if not (nn > 0.0 and math.isfinite(nn)):
                continue
            w = int(confs[k][py, px]) / 255.0
            if p is not None:
                dot = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
                r2 = (dot * dot) / nn
                w = w * (s2 / (s2 + r2))
            g = w / nn
            for j, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                m[j] = m[j] + g * (n[r] * n[c])
            ws = ws + w
            cnt += 1
        M[i], wsum[i], count[i] = m, ws, cnt
    return M, wsum, count


# ---- planes and points for the equality cases ------------------------------------------------------------------------------
def random_planes(views, seed=0, density=0.8):
    """(masks, orients, confs): masks with about `density` set, every orientation byte, confidences 0..255 with a share of zeros."""
    rng = np.random.default_rng(seed)
    masks = CC.random_masks(views, density, seed=seed)
    orients = [rng.integers(0, 256, (v.H, v.W), dtype=np.uint8) for v in views]
    confs = [np.where(rng.random((v.H, v.W)) < 0.15, 0, rng.integers(0, 256, (v.H, v.W))).astype(np.uint8) for v in views]
    return masks, orients, confs


def equality_views(V):
    """V ring views of the two mixed sizes; from four views on, the last is the identity view of the border cases."""
    return CC.ring_views(V) if V < 4 else CC.ring_views(V - 1) + [CC.identity_view(*CC.SIZES[0])]


def equality_points(n, seed=8):
    """n points: the border points of the identity view (u = 0 seen, u = W not; NaN, Inf, zc <= 0), points behind the ring cameras
    and far outside every frame, then a normal cloud."""
    border, _ = CC.border_points(*CC.SIZES[0])
    behind = np.array([[4.0, 0.0, 0.0], [0.0, 5.0, 0.2], [-6.0, 1.0, 0.3], [0.0, 0.0, 50.0], [0.0, 0.0, -50.0]])
    return np.ascontiguousarray(np.concatenate([border, behind, CC.cloud(max(n, 1), seed=seed)])[:n])


def unit_prev(n, seed=3, zero_every=7):
    """Unit vectors [n, 3], every zero_every-th one the zero vector (those points take the plain weight)."""
    p = np.random.default_rng(seed).normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p[::zero_every] = 0.0
    return p


# ---- the geometry rig ------------------------------------------------------------------------------------------------------
def rig(V, n, seed=0, W=64, H=64, f=70.0, radius=3.0):
    """(views, points, directions): V cameras of one size and focal length on a ring of `radius` whose heights alternate widely (so
    that no line is close to every viewing plane), n points inside the frame of all of them and a random unit direction each."""
    from utils.carve import View
    views = []
    for k in range(V):
        a = 2.0 * np.pi * k / V + 0.2
        R, t = CC.look_at((radius * np.cos(a), radius * np.sin(a), (-1.8, 0.3, 2.0, -0.6)[k % 4]))
        views.append(View(R=R, t=t, fx=f, fy=f, cx=W / 2, cy=H / 2, W=W, H=H, name=f"rig_{k}.png"))
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.55, 0.55, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return views, pts, d


def image_angle_bytes(views, pts, d):
    """uint8 [V, N]: the rounded analytic image angle theta = atan2(du, dv) mod pi, in steps of pi/255, of the projection of the
    line through pts along d -- (du, dv) is the derivative of the pixel (u, v) along d.  Also returns all-in-frame [N]."""
    out = np.zeros((len(views), pts.shape[0]), np.uint8)
    inside = np.ones(pts.shape[0], bool)
    for k, v in enumerate(views):
        pc = pts @ v.R.T + v.t
        dc = d @ v.R.T
        du = v.fx * (dc[:, 0] * pc[:, 2] - pc[:, 0] * dc[:, 2]) / pc[:, 2] ** 2
        dv = v.fy * (dc[:, 1] * pc[:, 2] - pc[:, 1] * dc[:, 2]) / pc[:, 2] ** 2
        theta = np.mod(np.arctan2(du, dv), np.pi)
        out[k] = np.mod(np.rint(theta * 255.0 / np.pi), 256).astype(np.uint8)     # (255 is pi: the same line as 0)
        u, w = v.fx * pc[:, 0] / pc[:, 2] + v.cx, v.fy * pc[:, 1] / pc[:, 2] + v.cy
        inside &= (pc[:, 2] > 0) & (u >= 0) & (u < v.W) & (w >= 0) & (w < v.H)
    return out, inside


def angle_deg(d, truth):
    """Angle between lines, degrees [N]; 90 for a zero d."""
    c = np.abs((d * truth).sum(axis=1)) / np.maximum(np.linalg.norm(d, axis=1) * np.linalg.norm(truth, axis=1), 1e-300)
    return np.degrees(np.arccos(np.clip(c, 0.0, 1.0)))


def relative_gap(M):
    """(l1 - l0)/l2 of the moment matrices [N, 6] (0 where l2 is not > 0)."""
    from utils.lift import symmetric
    lam = np.linalg.eigvalsh(symmetric(M))
    with np.errstate(all="ignore"):
        return np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)


# ---- the rule that compares two solvers (GPU tests 2 and 5) -------------------------------------------------------------------
def compare_solves(M, dev, host, gap_floor=1e-6):
    """dev, host: (d, coherence) of the two solvers on the moments M of rows that are not rank-deficient by construction.  Zero rows
    must be the same rows; where the relative eigengap is at least gap_floor, 1 - |d_dev . d_host| <= 1e-12 and the coherences differ
    by at most 1e-9 (a perturbation of a few ulp of l2 over that gap turns the vector by about 1e-9 rad).  Returns the number of
    non-zero rows below the gap, which are only required to be unit vectors."""
    (dd, cd), (dh, ch) = dev, host
    zero_d, zero_h = ~dd.any(axis=1), ~dh.any(axis=1)
    assert np.array_equal(zero_d, zero_h)
    assert np.isfinite(dd).all() and np.isfinite(cd).all() and (cd[zero_d] == 0).all() and (ch[zero_h] == 0).all()
    live = ~zero_h
    assert np.allclose(np.linalg.norm(dd[live], axis=1), 1.0, rtol=0, atol=1e-12)
    tight = live & (relative_gap(M) >= gap_floor)
    if tight.any():
        dot = np.abs((dd[tight] * dh[tight]).sum(axis=1))
        worst_d, worst_c = float((1.0 - dot).max()), float(np.abs(cd[tight] - ch[tight]).max())
        print(f"{int(tight.sum())} rows above the gap: max 1 - |dot| = {worst_d:.3e}, max coherence difference = {worst_c:.3e}")
        assert worst_d <= 1e-12 and worst_c <= 1e-9
    return int((live & ~tight).sum())


# ---- orientation maps for the driver's scene ---------------------------------------------------------------------------------
def write_orientations(root, views, folder="orientations", seed=5):
    """Random orientation and confidence PNGs for a carve_cases.build_scene scene; returns (orients, confs)."""
    from PIL import Image as PILImage
    os.makedirs(os.path.join(root, folder), exist_ok=True)
    rng = np.random.default_rng(seed)
    orients, confs = [], []
    for v in views:
        o = rng.integers(0, 256, (v.H, v.W), dtype=np.uint8)
        c = rng.integers(0, 256, (v.H, v.W), dtype=np.uint8)
        stem = os.path.basename(v.name).split(".")[0]
        PILImage.fromarray(o).save(os.path.join(root, folder, f"{stem}_orientation.png"))
        PILImage.fromarray(c).save(os.path.join(root, folder, f"{stem}_confidence.png"))
        orients.append(o)
        confs.append(c)
    return orients, confs


def smooth_orientations(root, views, direction=(0.3, -0.5, 0.8), folder="orientations"):
    """Orientation PNGs of ONE world direction seen from every view (per pixel: the image angle of that direction at the point where
    the pixel's ray is closest to the origin), confidence 255: a scene whose lifted directions are well determined."""
    from PIL import Image as PILImage
    os.makedirs(os.path.join(root, folder), exist_ok=True)
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    orients, confs = [], []
    for v in views:
        xs = (np.arange(v.W) + 0.5 - v.cx) / v.fx
        ys = (np.arange(v.H) + 0.5 - v.cy) / v.fy
        X, Y = np.meshgrid(xs, ys)
        zc = float(np.linalg.norm(v.t))
        dc = v.R @ d
        du = v.fx * (dc[0] * zc - X * zc * dc[2]) / zc ** 2
        dv = v.fy * (dc[1] * zc - Y * zc * dc[2]) / zc ** 2
        o = np.mod(np.rint(np.mod(np.arctan2(du, dv), np.pi) * 255.0 / np.pi), 256).astype(np.uint8)
        c = np.full((v.H, v.W), 255, np.uint8)
        stem = os.path.basename(v.name).split(".")[0]
        PILImage.fromarray(o).save(os.path.join(root, folder, f"{stem}_orientation.png"))
        PILImage.fromarray(c).save(os.path.join(root, folder, f"{stem}_confidence.png"))
        orients.append(o)
        confs.append(c)
    return orients, confs, d
