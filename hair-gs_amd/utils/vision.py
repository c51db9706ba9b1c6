"""Orientation maps of input views: the reference's utils/vision.py estimate_orientation_field, which its dataset parsers use to
write orientations/<stem>_orientation.png and <stem>_confidence.png, restated without cv2 (not installed where this project runs).

The contract (DESIGN.md "Orientation maps"):
  1. gray: a 2-D uint8 image as it is; H x W x 3 uint8 RGB through OpenCV's 8-bit RGB2GRAY, (4899 R + 9617 G + 1868 B + 8192) >> 14;
     H x W x 4 drops alpha.  Other dtypes raise TypeError (every reference call site passes uint8).
  2. kernels: thetas = np.linspace(0, pi, num_angles) (theta = pi repeats theta = 0); each kernel is cv2.getGaborKernel((ks, ks),
     sigma, theta, lambda_, gamma, psi=0, CV_32F), side 2 (ks // 2) + 1, evaluated here in float64 and stored as float32.
  3. responses: cv2.filter2D(gray, -1, k): a correlation anchored at the kernel centre, BORDER_REFLECT_101, saturated to uint8
     (round half to even, clamp to [0, 255]; negative responses become 0, so the reference's np.abs does nothing).
  4. orientation: the first argmax over the angles; field = thetas[idx] (float64).
  5. confidence: var = sum_k (d_k d_k) r_k / (sum_k r_k + 1e-7), d_k = pi/2 - | |theta* - theta_k| - pi/2 |, summed in plain k order;
     conf = (1 / var^2) / max over the view's var != 0 pixels, 1 elsewhere, float32.  A view without any var != 0 pixel raises
     ValueError, as the reference's np.max of an empty array does.
What is not pinned, since cv2 cannot be run: OpenCV's own accumulation precision in filter2D (here: float64, exact products), its
libm's exp / cos in getGaborKernel (here: numpy's; a float32 kernel value may differ in the last place), and numpy's pairwise
order of the reference's sum over k (here: plain k order on both backends, which agree bit for bit; the reference can differ in
the last ulp of var).

Two backends: device=None (or "cpu") correlates with scipy.signal.fftconvolve per angle in float64 and keeps only the uint8
stack; device="cuda" runs csrc/hgs_vision.hip (float64 FMA accumulation).  Their uint8 responses agree except where the exact
correlation lies within ~1e-9 of a half-integer, and from equal responses they compute equal fields and confidences."""
import numpy as np

__all__ = ["gabor_kernels", "to_gray", "estimate_orientation_field", "estimate_orientation_fields", "orientation_pngs",
           "NoVarianceError", "DEVICE_MAX_ANGLES", "DEVICE_MAX_SIDE"]

DEVICE_MAX_ANGLES = 256   # the device path stores the angle index as a byte
DEVICE_MAX_SIDE = 63      # kernel side (kernel_size <= 63)


def gabor_kernels(kernel_size=31, sigma=2, lambda_=3, gamma=0.5, num_angles=180):
    """(thetas float64 [A], kernels float32 [A, side, side]) as cv2.getGaborKernel builds them (psi = 0, CV_32F): xmax = ymax =
    kernel_size // 2, value(x, y) stored at [ymax - y, xmax - x]."""
    ks = int(kernel_size)
    if ks < 1:
        raise ValueError(f"kernel_size must be >= 1, got {kernel_size}")
    if int(num_angles) < 1:
        raise ValueError(f"num_angles must be >= 1, got {num_angles}")
    thetas = np.linspace(0, np.pi, int(num_angles))
    half = ks // 2
    sx, sy = float(sigma), float(sigma) / float(gamma)
    ex, ey = -0.5 / (sx * sx), -0.5 / (sy * sy)
    cscale = np.pi * 2 / float(lambda_)
    y, x = np.meshgrid(np.arange(-half, half + 1, dtype=np.float64), np.arange(-half, half + 1, dtype=np.float64), indexing="ij")
    kernels = np.empty((len(thetas), 2 * half + 1, 2 * half + 1), np.float32)
    for a, th in enumerate(thetas):
        c, s = np.cos(th), np.sin(th)
        xr = x * c + y * s
        yr = -x * s + y * c
        v = np.exp(ex * xr * xr + ey * yr * yr) * np.cos(cscale * xr)
        kernels[a] = v[::-1, ::-1]            # [ymax - y, xmax - x]
    return thetas, kernels


def to_gray(image):
    """uint8 [H, W] from a uint8 [H, W], [H, W, 3] (RGB) or [H, W, 4] (RGBA, alpha dropped) image (OpenCV's 8-bit RGB2GRAY)."""
    image = np.asarray(image)
    if image.dtype != np.uint8:
        raise TypeError(f"estimate_orientation_field takes uint8 images, got {image.dtype}")
    if image.ndim == 2:
        return image
    if image.ndim == 3 and image.shape[2] in (3, 4):
        rgb = image[..., :3].astype(np.int32)
        return ((4899 * rgb[..., 0] + 9617 * rgb[..., 1] + 1868 * rgb[..., 2] + 8192) >> 14).astype(np.uint8)
    raise ValueError(f"expected an [H, W], [H, W, 3] or [H, W, 4] image, got shape {image.shape}")


def _pre_rounding(gray, kernel):
    """float64 [H, W]: the correlation of gray with one kernel, anchor at the centre, BORDER_REFLECT_101 (np.pad "reflect"
    repeats the reflection where the view is narrower than the half-width)."""
    from scipy.signal import fftconvolve
    half = kernel.shape[0] // 2
    padded = np.pad(gray.astype(np.float64), half, mode="reflect")
    return fftconvolve(padded, kernel[::-1, ::-1].astype(np.float64), mode="valid")


def _saturate(r):
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def _cpu_responses(gray, kernels, near=None):
    """uint8 [A, H, W] responses; with near = eps also the [H, W] mask of pixels where some pre-rounding response lies within eps
    of a half-integer (where float64 rounding of a different summation order may round the other way)."""
    stack = np.empty((len(kernels),) + gray.shape, np.uint8)
    mask = np.zeros(gray.shape, bool) if near is not None else None
    for a, k in enumerate(kernels):
        r = _pre_rounding(gray, k)
        stack[a] = _saturate(r)
        if near is not None:
            mask |= np.abs(r - np.floor(r) - 0.5) <= near
    return stack, mask


def _pre_rounding_responses(gray, kernel_size=31, sigma=2, lambda_=3, gamma=0.5, num_angles=180):
    """float64 [A, H, W]: the CPU path's responses before rounding (small views: tests, diagnosis)."""
    _, kernels = gabor_kernels(kernel_size, sigma, lambda_, gamma, num_angles)
    return np.stack([_pre_rounding(to_gray(gray), k) for k in kernels])


def _cpu_near_boundary(gray, kernel_size=31, sigma=2, lambda_=3, gamma=0.5, num_angles=180, eps=1e-6):
    """[H, W] bool: pixels where some CPU pre-rounding response lies within eps of a half-integer."""
    _, kernels = gabor_kernels(kernel_size, sigma, lambda_, gamma, num_angles)
    return _cpu_responses(to_gray(gray), kernels, near=eps)[1]


def _field_variance(stack, thetas):
    """(idx [H, W], var float64 [H, W]) from the uint8 responses [A, H, W]: first argmax, then the variance in plain k order."""
    idx = np.argmax(stack, axis=0)
    th = thetas[idx]
    acc = np.zeros(th.shape, np.float64)
    for k in range(len(thetas)):
        d = np.pi / 2 - np.abs(np.abs(th - thetas[k]) - np.pi / 2)
        acc += (d * d) * stack[k]
    var = acc / (stack.sum(axis=0, dtype=np.int64) + 1e-7)
    return idx, var


def _confidence(var, what="the view"):
    has = var != 0
    if not has.any():
        raise ValueError(f"{what} has no pixel with nonzero orientation variance (a uniform image?): the confidence is undefined")
    inv = 1 / (var * var)[has]
    conf = np.ones(var.shape, np.float32)
    conf[has] = inv / inv.max()
    return conf


class NoVarianceError(ValueError):
    """Views (their positions in the batch) without a pixel of nonzero orientation variance: their confidence is undefined."""

    def __init__(self, views):
        self.views = list(views)
        super().__init__(f"view(s) {self.views} of the batch have no pixel with nonzero orientation variance (a uniform image?): "
                         "the confidence is undefined")


def _device_limits(kernel_size, num_angles):
    side = 2 * (int(kernel_size) // 2) + 1
    if not (2 <= int(num_angles) <= DEVICE_MAX_ANGLES):
        raise ValueError(f"the device path needs 2 <= num_angles <= {DEVICE_MAX_ANGLES}, got {num_angles}")
    if not (1 <= int(kernel_size) and side <= DEVICE_MAX_SIDE):
        raise ValueError(f"the device path needs 1 <= kernel_size <= {DEVICE_MAX_SIDE}, got {kernel_size}")


def estimate_orientation_fields(gray, kernel_size=31, sigma=2, lambda_=3, gamma=0.5, num_angles=180, return_responses=False):
    """Batched device form: gray = uint8 tensor [N, H, W] on a CUDA(HIP) device -> (field float64 [N, H, W], confidence float32
    [N, H, W]) device tensors (+ the uint8 responses [N, H, W, A] with return_responses).  The confidence is normalised per view.
    Raises ValueError before any launch when num_angles or kernel_size is outside the device limits, and NoVarianceError (a
    ValueError naming the batch positions) after the run when a view has no pixel with nonzero variance."""
    import torch
    import hgs_runtime as rt
    _device_limits(kernel_size, num_angles)
    if not isinstance(gray, torch.Tensor) or gray.dtype != torch.uint8 or gray.dim() != 3:
        raise TypeError("estimate_orientation_fields takes a uint8 tensor [N, H, W]")
    gray = rt.require_gpu_tensor(gray, "gray", torch.uint8)
    N, H, W = gray.shape
    thetas, kernels = gabor_kernels(kernel_size, sigma, lambda_, gamma, num_angles)
    A, side = kernels.shape[0], kernels.shape[1]
    dev = gray.device
    th = torch.from_numpy(thetas).to(dev)
    w = torch.from_numpy(kernels.astype(np.float64)).to(dev)
    idx = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    var = torch.empty((N, H, W), dtype=torch.float64, device=dev)
    maxinv = torch.empty(N, dtype=torch.float64, device=dev)
    conf = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    resp = torch.empty((N, H, W, A), dtype=torch.uint8, device=dev) if return_responses else None
    L = rt.lib()
    scratch = torch.empty(int(L.hgs_orientation_scratch_bytes(N, H, W, A, side)), dtype=torch.uint8, device=dev)
    s = rt.current_stream()
    rt.check(L.hgs_orientation_field(s, N, H, W, rt.ptr(gray), A, side, rt.ptr(w), rt.ptr(th), rt.ptr(idx), rt.ptr(var),
                                     rt.ptr(maxinv), rt.ptr(resp), rt.ptr(scratch), scratch.numel()))
    rt.check(L.hgs_orientation_confidence(s, N, H, W, rt.ptr(var), rt.ptr(maxinv), rt.ptr(conf)))
    flat = (maxinv == 0).nonzero().flatten().tolist()
    if flat:
        raise NoVarianceError(flat)
    field = th[idx.long()]
    return (field, conf, resp) if return_responses else (field, conf)


def estimate_orientation_field(image, kernel_size=31, sigma=2, lambda_=3, gamma=0.5, num_angles=180, device=None):
    """Orientation field (float64 [H, W], radians in [0, pi]) and confidence (float32 [H, W], in (0, 1]) of one uint8 image, the
    reference's signature and result (module docstring: the contract).  device=None or "cpu": the CPU path (scipy FFT
    correlation per angle); device="cuda": the HIP kernels."""
    gray = to_gray(image)
    if device is None or str(device) == "cpu":
        thetas, kernels = gabor_kernels(kernel_size, sigma, lambda_, gamma, num_angles)
        stack, _ = _cpu_responses(gray, kernels)
        idx, var = _field_variance(stack, thetas)
        return thetas[idx], _confidence(var)
    import torch
    _device_limits(kernel_size, num_angles)
    g = torch.from_numpy(np.ascontiguousarray(gray)).to(device)[None]
    field, conf = estimate_orientation_fields(g, kernel_size, sigma, lambda_, gamma, num_angles)
    return field[0].cpu().numpy(), conf[0].cpu().numpy()


def orientation_pngs(field, conf):
    """The two uint8 images the reference's parsers write: orientation = field * 255 / pi and confidence = conf * 255, truncated."""
    field, conf = np.asarray(field), np.asarray(conf)
    return (field * 255 / np.pi).astype(np.uint8), (conf * 255).astype(np.uint8)
