"""Undistortion of a COLMAP capture: the camera models with radial / tangential distortion, the pinhole camera an undistorted view
gets, and the warp of the images and masks into it (undistort.py is the scene driver; the reference leaves this step to COLMAP's
image_undistorter, whose rule this module restates -- parity with COLMAP's binary is not pinned by execution).

The contract (this module's numpy path, csrc/hgs_undistort.hip and the tests' loop restatement state the same thing).  Every
operation is float64 with one rounding each, in exactly the order written (the kernel is built with -ffp-contract=off).

Models.  (u, v) are normalised pinhole coordinates; uu = u*u, vv = v*v, r2 = uu + vv.
    SIMPLE_PINHOLE (f, cx, cy), PINHOLE (fx, fy, cx, cy)         du = dv = 0
    SIMPLE_RADIAL (f, cx, cy, k)                                rad = k*r2
    RADIAL (f, cx, cy, k1, k2), OPENCV (fx, fy, cx, cy, k1, k2, p1, p2)
                                                                rad = k1*r2 + k2*(r2*r2)
    FULL_OPENCV (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6)   r4 = r2*r2, r6 = r4*r2,
                                                                rad = (((1 + k1*r2) + k2*r4) + k3*r6) / (((1 + k4*r2) + k5*r4) + k6*r6) - 1
    du = u*rad, dv = v*rad, and for the two OPENCV models, with uv = u*v:
    du = (du + (2*p1)*uv) + p2*(r2 + 2*uu),  dv = (dv + (2*p2)*uv) + p1*(r2 + 2*vv)
    img_from_cam:  x = fx*(u + du) + cx,  y = fy*(v + dv) + cy      (single-focal models: fx = fy = f)
The fisheye, FOV and thin-prism models need atan, which no two of the three statements would round alike: they are refused by name.

cam_from_img (host only: the border scan and the keypoints): Newton's iteration on (u + du, v + dv) = ((x - cx)/fx, (y - cy)/fy)
from that point, NEWTON_ITERATIONS steps with the analytic Jacobian; a step whose Jacobian is singular or not finite is skipped.

Output camera, undistorted_camera(camera, blank_pixels, min_scale, max_scale): PINHOLE with the source's fx, fy, cx, cy; the pixel
centres of the four borders -- (0.5, y + 0.5), (W - 0.5, y + 0.5) for every row, (x + 0.5, 0.5), (x + 0.5, H - 0.5) for every column
-- are undistorted (fx*u + cx, fy*v + cy);
    min_scale_x = min(cx/(cx - min left x), (W - 0.5 - cx)/(max right x - cx))
    max_scale_x = max(cx/(cx - max left x), (W - 0.5 - cx)/(min right x - cx))
    scale_x = 1/(min_scale_x*blank + max_scale_x*(1 - blank)) clamped to [min_scale, max_scale]
    W' = max(1, int(scale_x*W)),  cx' = cx*W'/W                  (and likewise for y: top / bottom, H, cy)
blank_pixels = 0 keeps the largest view without a blank pixel, 1 the smallest that loses no source pixel.  A camera without
distortion -- a pinhole model, or every coefficient 0 -- keeps its size and principal point: the scan would take a pixel off it,
since cx/(cx - 0.5) is not 1 where (W - 0.5 - cx)/(W - 0.5 - cx) is.

Warp, undistort_images(images [N, H, W, C] uint8, camera, out_camera, mode): for the output pixel (x, y)
    u = ((x + 0.5) - cx')/fx',  v = ((y + 0.5) - cy')/fy';  (sx, sy) = img_from_cam(u, v) - 0.5
    valid iff 0 <= sx <= W - 1 and 0 <= sy <= H - 1               (a NaN is invalid)
    x0 = floor(sx), x1 = min(x0 + 1, W - 1), wx = sx - x0, and likewise for y
    value = (1 - wy)*((1 - wx)*p00 + wx*p01) + wy*((1 - wx)*p10 + wx*p11)        (pRC: row y_R, column x_C)
    mode "bilinear":  floor(value + 0.5);  mode "threshold" (masks): 255 where value >= 127.5, else 0;  0 where invalid.
(The loader truncates mask/255 to bool: a bilinear mask would lose a pixel along every edge.)  The [H', W'] validity plane is
returned as well.  (COLMAP's bitmap interpolation has a bounds test of its own, which is not restated: the rule above is this
project's.)  There is no region of interest and no max_image_size.

device=None: numpy.  device="cuda": hgs_undistort_images, whose bytes and validity plane are the numpy path's.  The caller chooses;
neither falls back to the other (the convention of utils/normals.py and scene/strand_export.py)."""
import numpy as np

from data.colmap import CAMERA_MODEL_NAMES, Camera

NEWTON_ITERATIONS = 20
MODES = {"bilinear": 0, "threshold": 1}
SUPPORTED = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
CHANNELS = (1, 3, 4)


class Intrinsics:
    """A camera's parameters by name: fx, fy, cx, cy, k1..k6, p1, p2 (those the model lacks are 0)."""
    __slots__ = ("model", "fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2")

    def __init__(self, camera):
        if camera.model not in CAMERA_MODEL_NAMES:
            raise ValueError(f"unknown camera model {camera.model}")
        if camera.model not in SUPPORTED:
            raise ValueError(f"camera model {camera.model} is not supported: the undistortion covers {', '.join(SUPPORTED)} "
                             "(the fisheye, FOV and thin-prism models need atan)")
        p = [float(v) for v in np.asarray(camera.params, np.float64).reshape(-1)]
        if len(p) != CAMERA_MODEL_NAMES[camera.model].num_params:
            raise ValueError(f"camera model {camera.model} takes {CAMERA_MODEL_NAMES[camera.model].num_params} parameters, got {len(p)}")
        self.model = camera.model
        self.k1 = self.k2 = self.k3 = self.k4 = self.k5 = self.k6 = self.p1 = self.p2 = 0.0
        if camera.model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL"):
            self.fx = self.fy = p[0]
            self.cx, self.cy = p[1], p[2]
            if camera.model == "SIMPLE_RADIAL":
                self.k1 = p[3]
            elif camera.model == "RADIAL":
                self.k1, self.k2 = p[3], p[4]
        else:
            self.fx, self.fy, self.cx, self.cy = p[0], p[1], p[2], p[3]
            if camera.model in ("OPENCV", "FULL_OPENCV"):
                self.k1, self.k2, self.p1, self.p2 = p[4], p[5], p[6], p[7]
            if camera.model == "FULL_OPENCV":
                self.k3, self.k4, self.k5, self.k6 = p[8], p[9], p[10], p[11]


def is_pinhole(camera):
    return camera.model in ("SIMPLE_PINHOLE", "PINHOLE")


def has_distortion(camera):
    """False for the pinhole models and for a camera whose distortion coefficients are all 0."""
    I = camera if isinstance(camera, Intrinsics) else Intrinsics(camera)
    return any(c != 0.0 for c in (I.k1, I.k2, I.k3, I.k4, I.k5, I.k6, I.p1, I.p2))


def _distortion(I, u, v):
    """(du, dv) of float64 arrays, in the contract's operation order."""
    if I.model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return np.zeros_like(u), np.zeros_like(v)
    uu, vv = u * u, v * v
    r2 = uu + vv
    if I.model == "SIMPLE_RADIAL":
        rad = I.k1 * r2
    elif I.model == "FULL_OPENCV":
        r4 = r2 * r2
        r6 = r4 * r2
        with np.errstate(divide="ignore", invalid="ignore"):
            rad = (((1.0 + I.k1 * r2) + I.k2 * r4) + I.k3 * r6) / (((1.0 + I.k4 * r2) + I.k5 * r4) + I.k6 * r6) - 1.0
    else:
        rad = I.k1 * r2 + I.k2 * (r2 * r2)
    du, dv = u * rad, v * rad
    if I.model in ("OPENCV", "FULL_OPENCV"):
        uv = u * v
        du = (du + (2.0 * I.p1) * uv) + I.p2 * (r2 + 2.0 * uu)
        dv = (dv + (2.0 * I.p2) * uv) + I.p1 * (r2 + 2.0 * vv)
    return du, dv


def _jacobian(I, u, v):
    """d(u + du, v + dv) / d(u, v): (j00, j01, j10, j11)."""
    r2 = u * u + v * v
    if I.model == "FULL_OPENCV":
        r4 = r2 * r2
        num = 1.0 + I.k1 * r2 + I.k2 * r4 + I.k3 * r4 * r2
        den = 1.0 + I.k4 * r2 + I.k5 * r4 + I.k6 * r4 * r2
        dnum = I.k1 + 2.0 * I.k2 * r2 + 3.0 * I.k3 * r4
        dden = I.k4 + 2.0 * I.k5 * r2 + 3.0 * I.k6 * r4
        rad, drad = num / den - 1.0, (dnum * den - num * dden) / (den * den)      # d rad / d r2
    else:
        rad, drad = I.k1 * r2 + I.k2 * r2 * r2, I.k1 + 2.0 * I.k2 * r2
    cross = 2.0 * u * v * drad + 2.0 * I.p1 * u + 2.0 * I.p2 * v
    return (1.0 + rad + 2.0 * u * u * drad + 2.0 * I.p1 * v + 6.0 * I.p2 * u, cross,
            cross, 1.0 + rad + 2.0 * v * v * drad + 2.0 * I.p2 * u + 6.0 * I.p1 * v)


def img_from_cam(camera, u, v):
    """Image coordinates (x, y) of the normalised points (u, v); float64 arrays of one shape."""
    I = camera if isinstance(camera, Intrinsics) else Intrinsics(camera)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    du, dv = _distortion(I, u, v)
    return I.fx * (u + du) + I.cx, I.fy * (v + dv) + I.cy


def cam_from_img(camera, x, y):
    """Normalised points (u, v) of the image coordinates (x, y): NEWTON_ITERATIONS Newton steps, vectorised over the points."""
    I = camera if isinstance(camera, Intrinsics) else Intrinsics(camera)
    tx, ty = (np.asarray(x, np.float64) - I.cx) / I.fx, (np.asarray(y, np.float64) - I.cy) / I.fy
    if I.model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return tx, ty
    u, v = tx.copy(), ty.copy()
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_ITERATIONS):
            du, dv = _distortion(I, u, v)
            ex, ey = (u + du) - tx, (v + dv) - ty
            j00, j01, j10, j11 = _jacobian(I, u, v)
            det = j00 * j11 - j01 * j10
            su, sv = (j11 * ex - j01 * ey) / det, (j00 * ey - j10 * ex) / det
            ok = np.isfinite(su) & np.isfinite(sv)
            u, v = np.where(ok, u - su, u), np.where(ok, v - sv, v)
    return u, v


def undistorted_camera(camera, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """The PINHOLE camera (data.colmap.Camera, same id) of the undistorted view of `camera`; see the module docstring."""
    I = Intrinsics(camera)
    W, H = int(camera.width), int(camera.height)
    blank = float(blank_pixels)
    if not 0.0 <= blank <= 1.0:
        raise ValueError(f"blank_pixels = {blank_pixels} outside [0, 1]")
    if not 0.0 < float(min_scale) <= float(max_scale):
        raise ValueError(f"min_scale = {min_scale}, max_scale = {max_scale}: need 0 < min_scale <= max_scale")
    Wd, Hd, cx, cy = W, H, I.cx, I.cy
    if has_distortion(I):
        rows, cols = np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5
        left = I.fx * cam_from_img(I, np.full(H, 0.5), rows)[0] + I.cx
        right = I.fx * cam_from_img(I, np.full(H, W - 0.5), rows)[0] + I.cx
        top = I.fy * cam_from_img(I, cols, np.full(W, 0.5))[1] + I.cy
        bottom = I.fy * cam_from_img(I, cols, np.full(W, H - 0.5))[1] + I.cy

        def scale(c, size, lo, hi):
            mn = min(c / (c - lo.min()), (size - 0.5 - c) / (hi.max() - c))
            mx = max(c / (c - lo.max()), (size - 0.5 - c) / (hi.min() - c))
            s = 1.0 / (mn * blank + mx * (1.0 - blank))
            return min(max(s, float(min_scale)), float(max_scale))
        Wd, Hd = max(1, int(scale(I.cx, W, left, right) * W)), max(1, int(scale(I.cy, H, top, bottom) * H))
        cx, cy = I.cx * Wd / W, I.cy * Hd / H
    return Camera(id=camera.id, model="PINHOLE", width=Wd, height=Hd, params=np.array([I.fx, I.fy, cx, cy], np.float64))


def _pinhole(out_camera):
    if out_camera.model != "PINHOLE":
        raise ValueError(f"the output camera must be PINHOLE, got {out_camera.model}")
    fx, fy, cx, cy = (float(v) for v in out_camera.params)
    return fx, fy, cx, cy


def undistort_keypoints(xys, camera, out_camera):
    """Keypoints [n, 2] of the source image (COLMAP's convention: a pixel's centre is at + 0.5) in the undistorted image."""
    fx, fy, cx, cy = _pinhole(out_camera)
    xys = np.asarray(xys, np.float64).reshape(-1, 2)
    u, v = cam_from_img(camera, xys[:, 0], xys[:, 1])
    return np.column_stack([fx * u + cx, fy * v + cy])


def source_map(camera, out_camera):
    """(sx, sy, valid) [H', W']: where every output pixel samples the source, and whether it may."""
    I = Intrinsics(camera)
    fx, fy, cx, cy = _pinhole(out_camera)
    W, H = int(camera.width), int(camera.height)
    u = ((np.arange(int(out_camera.width), dtype=np.float64) + 0.5) - cx) / fx
    v = ((np.arange(int(out_camera.height), dtype=np.float64) + 0.5) - cy) / fy
    x, y = img_from_cam(I, *np.meshgrid(u, v))
    sx, sy = x - 0.5, y - 0.5
    with np.errstate(invalid="ignore"):
        valid = (sx >= 0.0) & (sx <= W - 1) & (sy >= 0.0) & (sy <= H - 1)
    return sx, sy, valid


def _check_images(images, camera, mode):
    if mode not in MODES:
        raise ValueError(f"mode = {mode!r}: 'bilinear' or 'threshold'")
    if images.ndim != 4 or tuple(images.shape[1:3]) != (int(camera.height), int(camera.width)) or images.shape[3] not in CHANNELS:
        raise ValueError(f"images of shape {tuple(images.shape)}: [N, {camera.height}, {camera.width}, C] with C in {CHANNELS} expected")
    if images.shape[0] < 1:
        raise ValueError("no image to undistort")


def undistort_numpy(images, camera, out_camera, mode):
    _check_images(images, camera, mode)
    if images.dtype != np.uint8:
        raise TypeError(f"images must be uint8, got {images.dtype}")
    N, H, W, C = images.shape
    sx, sy, valid = source_map(camera, out_camera)
    sxv, syv = sx[valid], sy[valid]
    x0, y0 = np.floor(sxv).astype(np.int64), np.floor(syv).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx, wy = (sxv - x0)[:, None], (syv - y0)[:, None]
    omx, omy = 1.0 - wx, 1.0 - wy
    out = np.zeros((N,) + valid.shape + (C,), np.uint8)
    for n in range(N):
        img = images[n]
        value = omy * (omx * img[y0, x0].astype(np.float64) + wx * img[y0, x1].astype(np.float64)) \
            + wy * (omx * img[y1, x0].astype(np.float64) + wx * img[y1, x1].astype(np.float64))
        out[n][valid] = np.floor(value + 0.5).astype(np.uint8) if mode == "bilinear" else np.where(value >= 127.5, 255, 0).astype(np.uint8)
    return out, valid


def undistort_device(images, camera, out_camera, mode, want_valid=True):
    """hgs_undistort_images on a resident uint8 tensor [N, H, W, C]: (out [N, H', W', C] uint8, valid [H', W'] bool or None), both
    on the tensor's device."""
    import torch
    import hgs_runtime as rt
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise TypeError("undistort_device takes a uint8 tensor [N, H, W, C]")
    _check_images(images, camera, mode)
    Intrinsics(camera)
    src = rt.require_gpu_tensor(images, "images", torch.uint8)
    N, H, W, C = src.shape
    Hd, Wd = int(out_camera.height), int(out_camera.width)
    params = np.zeros(12, np.float64)
    raw = np.asarray(camera.params, np.float64).reshape(-1)
    params[:raw.size] = raw
    pinhole = np.array(_pinhole(out_camera), np.float64)
    out = torch.empty((N, Hd, Wd, C), dtype=torch.uint8, device=src.device)
    valid = torch.empty((Hd, Wd), dtype=torch.uint8, device=src.device) if want_valid else None
    with torch.cuda.device(src.device):
        rt.check(rt.lib().hgs_undistort_images(rt.current_stream(), N, C, H, W, Hd, Wd, CAMERA_MODEL_NAMES[camera.model].model_id,
                                               params.ctypes.data, pinhole.ctypes.data, rt.ptr(src), rt.ptr(out), rt.ptr(valid),
                                               MODES[mode]))
    return out, (valid.to(torch.bool) if want_valid else None)


def undistort_images(images, camera, out_camera, mode="bilinear", device=None):
    """images [N, H, W, C] uint8 (host array) seen through `camera` -> (out [N, H', W', C] uint8, valid [H', W'] bool) in
    `out_camera` (undistorted_camera), host arrays.  device=None: numpy; "cuda": the HIP kernel, copies included."""
    images = np.ascontiguousarray(images)
    if device is None:
        return undistort_numpy(images, camera, out_camera, mode)
    if not str(device).startswith("cuda"):
        raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernel)")
    import torch
    if images.dtype != np.uint8:
        raise TypeError(f"images must be uint8, got {images.dtype}")
    out, valid = undistort_device(torch.from_numpy(images).to(device), camera, out_camera, mode)
    return out.cpu().numpy(), valid.cpu().numpy()
