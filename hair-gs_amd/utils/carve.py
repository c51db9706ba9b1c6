"""A Stage-I point cloud carved from a capture's hair masks: a voxel grid (or a cloud of points) is tested against the mask of every
calibrated view, and a point is kept where enough of the views that have it in frame agree that it is hair (init_cloud.py is the
scene driver; the reference starts Stage I from COLMAP's points, or from the FLAME head's vertices on NeRSemble).

The contract (this module's numpy path, csrc/hgs_carve.hip and the tests' loop restatement state the same thing).  All arithmetic is
float64 with one rounding per operation, in exactly the order written (the kernel file is built with -ffp-contract=off).

View.  The View of utils/views.py; its mask is the uint8 [H, W] plane of masks/<name> converted to L.  Views may differ in size.

Vote of a point (x, y, z) in view k, with seen, px, py of utils/views.py's projection contract:
    hit   iff  seen and mask[py, px] != 0                   (the loader's rule: (mask/255).astype(bool))
mask_votes(points f64 [N, 3], views, masks, images=None) returns, over all views, seen[N] and hits[N] as int32 and, with images
(uint8 [H, W, 3]), rgb_sum[N, 3] as int32: the sum of the pixel (py, px) over the views that hit.  Integer sums: exact, and
independent of the order of the views.

Keep rule, with integers min_views >= 1 and 0 <= min_percent <= 100:
    kept  iff  seen >= min_views  and  100*hits >= min_percent*seen
A percentage of the views that have the point in frame, not a strict intersection: "seen" means inside the frustum, not unoccluded,
and on a 360-degree capture the head hides the far side's hair from half the ring.  min_percent = 100 is the classical visual hull;
the driver's default of 50 is a knob chosen for such captures, not a measured optimum.  The kernel may leave a voxel's view loop as
soon as the outcome is decided (with m misses so far and r views left, 100*m > (100 - min_percent)*(seen + r) can never recover);
the result does not depend on it.

Grid.  carve_grid(origin f64[3], h, (nx, ny, nz), views, masks, min_views, min_percent) returns occ, uint8 [nz, ny, nx]: 1 where the
voxel centre origin_k + (i_k + 0.5)*h is kept.  1 <= n_k <= 1024 and 1 <= V <= 4096; h is finite and positive.  Only the centre is
sampled: a structure thinner than a voxel, or a mask with holes finer than a voxel's footprint, is kept or lost by where the
centres happen to fall (dilate() widens the masks).

Shell.  shell(occ) returns uint8 of the same shape: 1 where occ is 1 and at least one of the six face neighbours is 0 or lies
outside the grid.

Automatic bounds, auto_bounds (host-side numpy around a 64^3 carve_grid): the camera centres are C = -R^T t; the cube is centred on
their mean and its half side is the largest distance of a centre from that mean; a COARSE^3 grid over the cube is carved with the
caller's rule; the box of the kept coarse voxels is padded by one coarse voxel on every side and clipped to the cube.  No coarse
voxel kept is an error ("no voxel is consistent with the masks").  fine_grid(lo, hi, grid): h = longest side / grid,
n_k = max(1, ceil(side_k / h)), origin = lo.  Known limit: a wisp thinner than a coarse voxel can fall outside the box (the driver's
--bounds overrides it).

Mask dilation.  dilate(mask, r) is the (2r+1)^2 maximum filter of the uint8 plane, exact: shifted maxima in numpy, max_pool2d on the
device (values 0..255 and a maximum: no rounding).  Host plumbing around the kernels, not part of them.

Thinning.  select(n, max_points): which of n kept voxels (init_cloud.py) or scalp samples (init_scalp.py) are written when there are
more than max_points.

device=None: numpy.  device="cuda": the kernels, on device tensors.  The caller chooses; neither falls back to the other (the
convention of utils/normals.py and scene/strand_export.py)."""
import math

import numpy as np

from utils.views import camera, check_views, is_cuda, pack, pixel, upload_points
from utils.views import MAX_VIEWS, Packed, View, view_of  # noqa: F401  (what the carving's callers reach through this module)

MAX_DIM = 1024
COARSE = 64


def check_rule(min_views, min_percent):
    if int(min_views) != min_views or int(min_percent) != min_percent or min_views < 1 or not 0 <= min_percent <= 100:
        raise ValueError(f"min_views = {min_views} (an integer >= 1), min_percent = {min_percent} (an integer, 0 to 100)")
    return int(min_views), int(min_percent)


def _check_grid(h, dims, error=ValueError):
    nx, ny, nz = (int(n) for n in dims)
    if min(nx, ny, nz) < 1 or max(nx, ny, nz) > MAX_DIM:
        raise error(f"a grid of {nx} x {ny} x {nz} voxels (1 to {MAX_DIM} per axis)")
    if not (math.isfinite(h) and h > 0.0):
        raise error(f"voxel size h = {h}")
    return nx, ny, nz


def keep(seen, hits, min_views, min_percent):
    """The keep rule on integer arrays (numpy or torch)."""
    return (seen >= min_views) & (100 * hits >= min_percent * seen)


def select(n, max_points):
    """Positions (ascending) of the kept voxels or samples that are written: all n, or floor(j*n/max_points) for j = 0..max_points - 1."""
    if n <= max_points:
        return np.arange(n, dtype=np.int64)
    return (np.arange(max_points, dtype=np.int64) * n) // max_points


# ---- numpy path ------------------------------------------------------------------------------------------------------
def votes_numpy(points, views, masks, images=None):
    points = np.asarray(points, np.float64).reshape(-1, 3)
    check_views(views, masks, images)
    N = points.shape[0]
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    seen, hits = np.zeros(N, np.int32), np.zeros(N, np.int32)
    rgb = np.zeros((N, 3), np.int32) if images is not None else None
    for k, view in enumerate(views):
        s, py, px = pixel(view, *camera(view, x, y, z))
        hit = s & (masks[k][py, px] != 0)
        seen += s
        hits += hit
        if rgb is not None:
            rgb += np.where(hit[:, None], images[k][py, px].astype(np.int32), 0)
    return (seen, hits, rgb) if images is not None else (seen, hits)


def centres(origin, h, dims):
    """Voxel centres per axis: origin_k + (i_k + 0.5)*h."""
    origin = np.asarray(origin, np.float64).reshape(3)
    return [origin[k] + (np.arange(int(dims[k]), dtype=np.float64) + 0.5) * float(h) for k in range(3)]


def grid_numpy(origin, h, dims, views, masks, min_views, min_percent):
    h = float(h)
    nx, ny, nz = _check_grid(h, dims)
    min_views, min_percent = check_rule(min_views, min_percent)
    check_views(views, masks)
    xs, ys, zs = centres(origin, h, (nx, ny, nz))
    occ = np.empty((nz, ny, nx), np.uint8)
    slab = max(1, (1 << 20) // (nx * ny))                       # z slices per pass: about 2^20 points
    for z0 in range(0, nz, slab):
        Z, Y, X = np.meshgrid(zs[z0:z0 + slab], ys, xs, indexing="ij")
        seen, hits = votes_numpy(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1), views, masks)
        occ[z0:z0 + slab] = keep(seen, hits, min_views, min_percent).reshape(Z.shape)
    return occ


def shell_numpy(occ):
    occ = np.asarray(occ)
    if occ.ndim != 3 or occ.dtype != np.uint8:
        raise ValueError("occ must be uint8 [nz, ny, nx]")
    full = np.zeros(tuple(n + 2 for n in occ.shape), bool)
    full[1:-1, 1:-1, 1:-1] = occ != 0
    inner = (full[:-2, 1:-1, 1:-1] & full[2:, 1:-1, 1:-1] & full[1:-1, :-2, 1:-1] & full[1:-1, 2:, 1:-1]
             & full[1:-1, 1:-1, :-2] & full[1:-1, 1:-1, 2:])
    return ((occ != 0) & ~inner).astype(np.uint8)


def dilate_numpy(mask, r):
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.dtype != np.uint8 or int(r) != r or r < 0:
        raise ValueError("dilate takes a uint8 [H, W] plane and an integer radius >= 0")
    out = mask.copy()
    for axis in (0, 1):                                          # the square window is separable
        src = out.copy()
        n = src.shape[axis]
        for d in range(1, min(int(r), n - 1) + 1):
            a, b = [slice(None)] * 2, [slice(None)] * 2
            a[axis], b[axis] = slice(0, n - d), slice(d, n)
            np.maximum(out[tuple(a)], src[tuple(b)], out=out[tuple(a)])
            np.maximum(out[tuple(b)], src[tuple(a)], out=out[tuple(b)])
    return out


# ---- device path -----------------------------------------------------------------------------------------------------
def votes_device(points, packed, with_rgb=False):
    """hgs_carve_votes on a float64 device tensor [N, 3]: (seen, hits) or (seen, hits, rgb_sum), int32 tensors on its device."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(points, "points", torch.float64)
    if points.dim() != 2 or points.shape[1] != 3:
        raise rt.HgsError(f"points of shape {tuple(points.shape)}: [N, 3] expected")
    if with_rgb and packed.images_dev is None:
        raise rt.HgsError("rgb_sum needs the views' images")
    V = rt.carve_check(packed.records, packed.views_dev, packed.masks_dev, packed.images_dev)
    N = points.shape[0]
    seen = torch.empty(N, dtype=torch.int32, device=points.device)
    hits = torch.empty(N, dtype=torch.int32, device=points.device)
    rgb = torch.empty((N, 3), dtype=torch.int32, device=points.device) if with_rgb else None
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_carve_votes(rt.current_stream(), N, rt.ptr(points), V, rt.ptr(packed.views_dev), rt.ptr(packed.masks_dev),
                                          rt.ptr(packed.images_dev) if with_rgb else None, rt.ptr(seen), rt.ptr(hits), rt.ptr(rgb)))
    return (seen, hits, rgb) if with_rgb else (seen, hits)


def grid_device(origin, h, dims, packed, min_views, min_percent):
    """hgs_carve_grid: occ, a uint8 tensor [nz, ny, nx] on the device of the packed views."""
    import torch
    import hgs_runtime as rt
    V = rt.carve_check(packed.records, packed.views_dev, packed.masks_dev, packed.images_dev)
    h = float(h)
    nx, ny, nz = _check_grid(h, dims, error=rt.HgsError)
    try:
        min_views, min_percent = check_rule(min_views, min_percent)
    except ValueError as e:
        raise rt.HgsError(str(e))
    origin = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(3))
    occ = torch.empty((nz, ny, nx), dtype=torch.uint8, device=packed.masks_dev.device)
    with torch.cuda.device(occ.device):
        rt.check(rt.lib().hgs_carve_grid(rt.current_stream(), origin.ctypes.data, h, nx, ny, nz, V, rt.ptr(packed.views_dev),
                                         rt.ptr(packed.masks_dev), min_views, min_percent, rt.ptr(occ)))
    return occ


def shell_device(occ):
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(occ, "occ", torch.uint8)
    if occ.dim() != 3:
        raise rt.HgsError("occ must be uint8 [nz, ny, nx]")
    nz, ny, nx = occ.shape
    _check_grid(1.0, (nx, ny, nz), error=rt.HgsError)
    out = torch.empty_like(occ)
    with torch.cuda.device(occ.device):
        rt.check(rt.lib().hgs_carve_shell(rt.current_stream(), nx, ny, nz, rt.ptr(occ), rt.ptr(out)))
    return out


def dilate_device(mask, r):
    """The (2r+1)^2 maximum filter of a uint8 device plane [H, W] (max_pool2d on float32: exact for 0..255)."""
    import torch
    if r == 0:
        return mask.clone()
    f = torch.nn.functional.max_pool2d(mask.to(torch.float32)[None, None], kernel_size=2 * int(r) + 1, stride=1, padding=int(r))
    return f[0, 0].to(torch.uint8)


# ---- host-array entry points -----------------------------------------------------------------------------------------
def mask_votes(points, views, masks, images=None, device=None):
    """(seen, hits) int32 [N], and rgb_sum int32 [N, 3] with images; host arrays."""
    if not is_cuda(device):
        return votes_numpy(points, views, masks, images)
    out = votes_device(upload_points(points, device), pack(views, masks, images, device), with_rgb=images is not None)
    return tuple(t.cpu().numpy() for t in out)


def carve_grid(origin, h, dims, views, masks, min_views, min_percent, device=None):
    """occ uint8 [nz, ny, nx], a host array."""
    if not is_cuda(device):
        return grid_numpy(origin, h, dims, views, masks, min_views, min_percent)
    return grid_device(origin, h, dims, pack(views, masks, None, device), min_views, min_percent).cpu().numpy()


def shell(occ, device=None):
    if not is_cuda(device):
        return shell_numpy(occ)
    import torch
    return shell_device(torch.from_numpy(np.ascontiguousarray(occ)).to(device)).cpu().numpy()


def dilate(mask, r, device=None):
    if not is_cuda(device):
        return dilate_numpy(mask, r)
    import torch
    if mask.ndim != 2 or mask.dtype != np.uint8 or int(r) != r or r < 0:
        raise ValueError("dilate takes a uint8 [H, W] plane and an integer radius >= 0")
    return dilate_device(torch.from_numpy(np.ascontiguousarray(mask)).to(device), int(r)).cpu().numpy()


# ---- bounds ----------------------------------------------------------------------------------------------------------
def camera_cube(views):
    """(lo f64[3], side): the cube centred on the mean camera centre C = -R^T t whose half side is the largest distance of a centre
    from that mean."""
    C = np.stack([-(np.asarray(v.R, np.float64).T @ np.asarray(v.t, np.float64)) for v in views])
    mean = C.mean(axis=0)
    half = float(np.linalg.norm(C - mean, axis=1).max())
    if not (math.isfinite(half) and half > 0.0):
        raise ValueError("the camera centres coincide: no cube to search (give the bounds)")
    return mean - half, 2.0 * half


def fine_grid(lo, hi, grid):
    """(origin, h, (nx, ny, nz)) of the box [lo, hi]: h = longest side / grid, n_k = max(1, ceil(side_k / h))."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    side = hi - lo
    if not (np.isfinite(side).all() and (side >= 0).all() and side.max() > 0 and int(grid) >= 1):
        raise ValueError(f"bounds {lo.tolist()} .. {hi.tolist()} with grid = {grid}")
    h = float(side.max()) / int(grid)
    return lo.copy(), h, tuple(max(1, int(math.ceil(float(s) / h))) for s in side)


def auto_bounds(views, masks, min_views, min_percent, device=None, carve=None):
    """(lo, hi) of the box to carve; `carve(origin, h, dims) -> occ host array` replaces carve_grid (the driver's packed views)."""
    cube_lo, side = camera_cube(views)
    hc = side / COARSE
    if carve is None:
        occ = carve_grid(cube_lo, hc, (COARSE,) * 3, views, masks, min_views, min_percent, device=device)
    else:
        occ = carve(cube_lo, hc, (COARSE,) * 3)
    iz, iy, ix = np.nonzero(occ)
    if ix.size == 0:
        raise ValueError("no voxel is consistent with the masks")
    first = np.array([ix.min(), iy.min(), iz.min()], np.float64) - 1.0
    last = np.array([ix.max(), iy.max(), iz.max()], np.float64) + 2.0
    lo = np.maximum(cube_lo + first * hc, cube_lo)
    hi = np.minimum(cube_lo + last * hc, cube_lo + side)
    return lo, hi
