"""Downscaling of a pinhole capture: the area average of its images, the thresholded average of its masks, the double-angle average of
its orientation / confidence pairs, and the camera and keypoints of the smaller view (rescale.py is the scene driver; the reference's
parsers write the size they want, and scene.scene.camera_from_info subsamples the hair planes -- this project states its own rule).

The contract (this module's numpy path, csrc/hgs_rescale.hip and the tests' loop restatement state the same thing).  Every operation
is float64 with one rounding each, in exactly the order written (the kernels are built with -ffp-contract=off).

Sizes.  A source plane is [H, W], the output [H', W'] with 1 <= W' <= W and 1 <= H' <= H; enlarging raises ValueError.

Footprint and weights.  Output column x covers lo = (x*W)/W' to hi = ((x + 1)*W)/W' (both products are exact integers, one division
each); i0 = floor(lo), Kx = (W + W' - 1)//W' + 1; for k = 0..Kx - 1 the source column is i = min(i0 + k, W - 1) and its weight
    wx = min(i0 + k + 1, hi) - max(i0 + k, lo),   replaced by 0 unless it is > 0.
Rows likewise with H, H', wy, Ky.

Sums.  Terms are visited row by row, ky outer and kx inner, w = wy*wx.  A zero-weight term adds exactly nothing (a kernel may skip
it).  With an integer factor every weight is 1 and every sum an exact integer.

Images, rescale_images(images [N, H, W, C] uint8, (W', H'), mode), C in 1, 3, 4, one sum per channel:  acc = acc + w*p, A = A + w;
    mode "average":    min(255, floor(acc/A + 0.5))
    mode "threshold":  255 where acc/A >= 127.5, else 0     (masks: the rule of utils/undistort.py, for its reason -- the loader
                                                             truncates mask/255 to bool, so a blended edge would erode)

Orientation pairs, rescale_orientation(angle, confidence [N, H, W] uint8, mask [N, H, W] uint8 or None, (W', H')).  The loader decodes
theta = t*pi/255, so bytes 0 and 255 are one direction, and an orientation is a line: it is averaged as its double-angle vector.
The host builds the tables once with numpy (orientation_tables) and every statement of the contract reads them; nothing else
evaluates a trigonometric function:
    C[t] = cos(2*pi*t/255), S[t] = sin(2*pi*t/255) for t = 0..255, entry 255 set to entry 0
    HC[j] = cos(2*pi*(j - 0.5)/255), HS[j] = sin(2*pi*(j - 0.5)/255) for j = 1..255, the half-step boundaries between the codes
Per term whose mask byte is not 0 (without a mask every pixel counts):
    g = w*c,  X = X + g*C[t],  Y = Y + g*S[t],  Am = Am + w
    confidence byte: 0 if Am == 0, else min(255, floor(sqrt(X*X + Y*Y)/Am + 0.5))  -- the mean confidence times the coherence of the
                     directions: pixels that disagree lower it, which is what a confidence is for
    angle byte:      0 if X == 0 and Y == 0, else (the number of j in 1..255 with V = (X, Y) at or past H[j]) mod 255 -- the nearest
                     code, never 255.  upper(x, y) means y > 0 or (y == 0 and x > 0); V is at or past H iff upper(V) != upper(H) and H
                     is the upper one, or the halves are equal and HC*Y - HS*X >= 0 (two products, one subtraction).  The boundaries
                     ascend, so the count may be found by bisection (8 steps).
A box of one repeated pair (t, c) comes back as (t mod 255, c); a floor rule would lose one off both bytes to the rounding of the
table's norm and of the cross product.

Camera and keypoints, rescaled_camera(camera, (W', H')): PINHOLE and SIMPLE_PINHOLE only (any other model: run undistort.py first).
COLMAP's Camera::Rescale:  fx' = fx*W'/W, cx' = cx*W'/W, fy' = fy*H'/H, cy' = cy*H'/H.  A SIMPLE_PINHOLE camera stays one where
W'*H == H'*W (f' = f*W'/W) and becomes PINHOLE where the two ratios differ.  Keypoints: x' = x*W'/W, y' = y*H'/H.

device=None: numpy.  device="cuda": hgs_rescale_images / hgs_rescale_orientation, whose bytes are the numpy path's.  The caller
chooses; neither falls back to the other (the convention of utils/undistort.py)."""
import numpy as np

from data.colmap import Camera

MODES = {"average": 0, "threshold": 1}
CHANNELS = (1, 3, 4)


def _size(size, W, H):
    Wd, Hd = int(size[0]), int(size[1])
    if Wd < 1 or Hd < 1:
        raise ValueError(f"an output of {Wd} x {Hd} pixels")
    if Wd > W or Hd > H:
        raise ValueError(f"an output of {Wd} x {Hd} pixels from a source of {W} x {H}: enlarging is not supported")
    return Wd, Hd


def footprint(S, D):
    """(index [K, D] int64, weight [K, D] float64) of the K = (S + D - 1)//D + 1 taps of every output index along an axis of S source
    and D output pixels."""
    x = np.arange(D, dtype=np.int64)
    lo, hi = (x * S).astype(np.float64) / float(D), ((x + 1) * S).astype(np.float64) / float(D)
    i0 = np.floor(lo)
    K = (S + D - 1) // D + 1
    k = np.arange(K, dtype=np.float64)[:, None]
    w = np.minimum((i0 + k) + 1.0, hi) - np.maximum(i0 + k, lo)
    w = np.where(w > 0.0, w, 0.0)
    return np.minimum(i0.astype(np.int64) + np.arange(K, dtype=np.int64)[:, None], S - 1), w


def orientation_tables():
    """float64 [4, 256]: C, S (entry 255 = entry 0) and HC, HS (entries 1..255; entry 0 is unused and 0)."""
    t = np.arange(256, dtype=np.float64)
    tab = np.zeros((4, 256), np.float64)
    tab[0], tab[1] = np.cos(2 * np.pi * t / 255), np.sin(2 * np.pi * t / 255)
    tab[0, 255], tab[1, 255] = tab[0, 0], tab[1, 0]
    j = t[1:]
    tab[2, 1:], tab[3, 1:] = np.cos(2 * np.pi * (j - 0.5) / 255), np.sin(2 * np.pi * (j - 0.5) / 255)
    return tab


def _check_images(images, mode):
    if mode not in MODES:
        raise ValueError(f"mode = {mode!r}: 'average' or 'threshold'")
    if images.ndim != 4 or images.shape[3] not in CHANNELS or 0 in images.shape[1:3]:
        raise ValueError(f"images of shape {tuple(images.shape)}: [N, H, W, C] with C in {CHANNELS} expected")
    if images.shape[0] < 1:
        raise ValueError("no image to rescale")


def rescale_numpy(images, size, mode):
    _check_images(images, mode)
    if images.dtype != np.uint8:
        raise TypeError(f"images must be uint8, got {images.dtype}")
    N, H, W, C = images.shape
    Wd, Hd = _size(size, W, H)
    ix, wx = footprint(W, Wd)
    iy, wy = footprint(H, Hd)
    out = np.empty((N, Hd, Wd, C), np.uint8)
    for n in range(N):
        acc, A = np.zeros((Hd, Wd, C), np.float64), np.zeros((Hd, Wd), np.float64)
        for ky in range(iy.shape[0]):
            rows = images[n][iy[ky]]
            for kx in range(ix.shape[0]):
                w = wy[ky][:, None] * wx[kx][None, :]
                if not w.any():
                    continue
                acc = acc + w[:, :, None] * rows[:, ix[kx]].astype(np.float64)
                A = A + w
        v = acc / A[:, :, None]
        out[n] = np.minimum(255.0, np.floor(v + 0.5)).astype(np.uint8) if mode == "average" else np.where(v >= 127.5, 255, 0).astype(np.uint8)
    return out


def _check_pairs(angle, conf, mask):
    if angle.ndim != 3 or angle.shape[0] < 1 or 0 in angle.shape[1:]:
        raise ValueError(f"orientation planes of shape {tuple(angle.shape)}: [N, H, W] expected")
    for name, a in (("confidence", conf), ("mask", mask)):
        if a is not None and tuple(a.shape) != tuple(angle.shape):
            raise ValueError(f"{name} planes of shape {tuple(a.shape)}, orientation planes of shape {tuple(angle.shape)}")


def _upper(x, y):
    return (y > 0.0) | ((y == 0.0) & (x > 0.0))


def _angle_codes(X, Y, tab):
    """The angle byte of every (X, Y): the boundary count by bisection (they ascend), mod 255."""
    HC, HS = tab[2], tab[3]
    HU = _upper(HC, HS)
    vu = _upper(X, Y)
    count = np.zeros(X.shape, np.int64)
    for b in (128, 64, 32, 16, 8, 4, 2, 1):
        j = count + b
        hu = HU[j]
        past = np.where(hu != vu, hu, HC[j] * Y - HS[j] * X >= 0.0)
        count = np.where(past, j, count)
    return np.where((X == 0.0) & (Y == 0.0), 0, count % 255).astype(np.uint8)


def rescale_orientation_numpy(angle, conf, mask, size):
    _check_pairs(angle, conf, mask)
    for name, a in (("orientation", angle), ("confidence", conf), ("mask", mask)):
        if a is not None and a.dtype != np.uint8:
            raise TypeError(f"{name} planes must be uint8, got {a.dtype}")
    N, H, W = angle.shape
    Wd, Hd = _size(size, W, H)
    ix, wx = footprint(W, Wd)
    iy, wy = footprint(H, Hd)
    tab = orientation_tables()
    out_t, out_c = np.empty((N, Hd, Wd), np.uint8), np.empty((N, Hd, Wd), np.uint8)
    for n in range(N):
        X, Y, Am = (np.zeros((Hd, Wd), np.float64) for _ in range(3))
        for ky in range(iy.shape[0]):
            rt, rc = angle[n][iy[ky]], conf[n][iy[ky]]
            rm = None if mask is None else mask[n][iy[ky]]
            for kx in range(ix.shape[0]):
                w = wy[ky][:, None] * wx[kx][None, :]
                if not w.any():
                    continue
                if rm is not None:
                    w = np.where(rm[:, ix[kx]] != 0, w, 0.0)
                t = rt[:, ix[kx]]
                g = w * rc[:, ix[kx]].astype(np.float64)
                X, Y, Am = X + g * tab[0][t], Y + g * tab[1][t], Am + w
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.minimum(255.0, np.floor(np.sqrt(X * X + Y * Y) / Am + 0.5))
        out_c[n] = np.where(Am == 0.0, 0.0, c).astype(np.uint8)
        out_t[n] = _angle_codes(X, Y, tab)
    return out_t, out_c


def rescale_device(images, size, mode):
    """hgs_rescale_images on a resident uint8 tensor [N, H, W, C]: out [N, H', W', C] uint8 on the tensor's device."""
    import torch
    import hgs_runtime as rt
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise TypeError("rescale_device takes a uint8 tensor [N, H, W, C]")
    _check_images(images, mode)
    src = rt.require_gpu_tensor(images, "images", torch.uint8)
    N, H, W, C = src.shape
    Wd, Hd = _size(size, W, H)
    out = torch.empty((N, Hd, Wd, C), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        rt.check(rt.lib().hgs_rescale_images(rt.current_stream(), N, C, H, W, Hd, Wd, rt.ptr(src), rt.ptr(out), MODES[mode]))
    return out


def rescale_orientation_device(angle, conf, mask, size, tables=None):
    """hgs_rescale_orientation on resident uint8 tensors [N, H, W] (mask: a tensor or None): (angle', confidence') [N, H', W'] uint8 on
    their device.  tables: orientation_tables() as a float64 device tensor, for a caller that launches more than once."""
    import torch
    import hgs_runtime as rt
    for name, a in (("angle", angle), ("conf", conf), ("mask", mask)):
        if a is not None and (not isinstance(a, torch.Tensor) or a.dtype != torch.uint8):
            raise TypeError(f"rescale_orientation_device takes uint8 tensors [N, H, W]: {name}")
    _check_pairs(angle, conf, mask)
    angle = rt.require_gpu_tensor(angle, "angle", torch.uint8)
    conf = rt.require_gpu_tensor(conf, "conf", torch.uint8)
    mask = None if mask is None else rt.require_gpu_tensor(mask, "mask", torch.uint8)
    N, H, W = angle.shape
    Wd, Hd = _size(size, W, H)
    if tables is None:
        tables = torch.from_numpy(orientation_tables()).to(angle.device)
    tables = rt.require_device_buffer(tables, "tables", torch.float64)
    if tables.numel() != 4 * 256:
        raise rt.HgsError(f"the orientation tables hold {tables.numel()} values, 4 x 256 expected")
    out_t = torch.empty((N, Hd, Wd), dtype=torch.uint8, device=angle.device)
    out_c = torch.empty((N, Hd, Wd), dtype=torch.uint8, device=angle.device)
    with torch.cuda.device(angle.device):
        rt.check(rt.lib().hgs_rescale_orientation(rt.current_stream(), N, H, W, Hd, Wd, rt.ptr(angle), rt.ptr(conf), rt.ptr(mask),
                                                  rt.ptr(tables), rt.ptr(out_t), rt.ptr(out_c)))
    return out_t, out_c


def _device(device):
    if device is not None and not str(device).startswith("cuda"):
        raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernels)")
    return device


def rescale_images(images, size, mode="average", device=None):
    """images [N, H, W, C] uint8 (host array) -> [N, H', W', C] uint8 (host array), size = (W', H').  device=None: numpy; "cuda": the
    HIP kernel, copies included."""
    images = np.ascontiguousarray(images)
    if _device(device) is None:
        return rescale_numpy(images, size, mode)
    import torch
    if images.dtype != np.uint8:
        raise TypeError(f"images must be uint8, got {images.dtype}")
    return rescale_device(torch.from_numpy(images).to(device), size, mode).cpu().numpy()


def rescale_orientation(angle, conf, mask, size, device=None):
    """angle, conf [N, H, W] uint8 and mask [N, H, W] uint8 or None (host arrays) -> (angle', confidence') [N, H', W'] uint8 (host
    arrays), size = (W', H').  device=None: numpy; "cuda": the HIP kernel, copies included."""
    angle, conf = np.ascontiguousarray(angle), np.ascontiguousarray(conf)
    mask = None if mask is None else np.ascontiguousarray(mask)
    if _device(device) is None:
        return rescale_orientation_numpy(angle, conf, mask, size)
    import torch
    for name, a in (("orientation", angle), ("confidence", conf), ("mask", mask)):
        if a is not None and a.dtype != np.uint8:
            raise TypeError(f"{name} planes must be uint8, got {a.dtype}")
    dev = lambda a: None if a is None else torch.from_numpy(a).to(device)   # noqa: E731
    out_t, out_c = rescale_orientation_device(dev(angle), dev(conf), dev(mask), size)
    return out_t.cpu().numpy(), out_c.cpu().numpy()


def rescaled_camera(camera, size):
    """The camera (data.colmap.Camera, same id) of `camera`'s view at size = (W', H'); see the module docstring."""
    if camera.model not in ("PINHOLE", "SIMPLE_PINHOLE"):
        raise ValueError(f"camera model {camera.model} is not supported: the rescaling covers PINHOLE and SIMPLE_PINHOLE "
                         "(run undistort.py first)")
    W, H = int(camera.width), int(camera.height)
    Wd, Hd = _size(size, W, H)
    p = [float(v) for v in np.asarray(camera.params, np.float64).reshape(-1)]
    if camera.model == "SIMPLE_PINHOLE" and Wd * H == Hd * W:
        return Camera(id=camera.id, model="SIMPLE_PINHOLE", width=Wd, height=Hd,
                      params=np.array([p[0] * Wd / W, p[1] * Wd / W, p[2] * Hd / H], np.float64))
    fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if camera.model == "SIMPLE_PINHOLE" else p
    return Camera(id=camera.id, model="PINHOLE", width=Wd, height=Hd,
                  params=np.array([fx * Wd / W, fy * Hd / H, cx * Wd / W, cy * Hd / H], np.float64))


def rescale_keypoints(xys, camera, out_camera):
    """Keypoints [n, 2] of the source image in the rescaled image."""
    xys = np.asarray(xys, np.float64).reshape(-1, 2)
    return np.column_stack([xys[:, 0] * int(out_camera.width) / int(camera.width), xys[:, 1] * int(out_camera.height) / int(camera.height)])
