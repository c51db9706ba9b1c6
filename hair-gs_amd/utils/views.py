"""The calibrated pinhole views of a capture: how a world point becomes a pixel of one and when it counts as seen (the only numpy
definition; csrc/hgs_pinhole.h is the device one), and the plumbing that carries views and their planes to the kernels.  The stages
that walk the views -- utils/carve.py, utils/lift.py, utils/scalp.py -- project through this module.

View.  A PINHOLE or SIMPLE_PINHOLE camera of the sparse model with its image's pose: R = qvec2rotmat(qvec) (world -> camera,
row-major), t = tvec, fx, fy, cx, cy (COLMAP's principal point, not the centred one the FoV cameras of training assume), W, H.  Any
other camera model is refused by name: undistort.py makes pinholes of them.  A view's planes (its mask, its orientation map, ...) are
uint8 [H, W]; views may differ in size.

The projection contract (these numpy functions, the kernels and the tests' loop restatements state the same thing).  All arithmetic
is float64 with one rounding per operation, in exactly the order written (the kernel files are built with -ffp-contract=off).  For a
point (x, y, z) in view k:
    xc = ((R00*x + R01*y) + R02*z) + tx        (yc, zc likewise, rows 1 and 2)                    camera(view, x, y, z)
    u  = fx*(xc/zc) + cx,   v = fy*(yc/zc) + cy                                                   image_point(view, xc, yc, zc)
    seen  iff  zc > 0  and  0 <= u < W  and  0 <= v < H     (any NaN: not seen)                   pixel(view, xc, yc, zc)
    px = floor(u), py = floor(v)
"seen" means inside the frustum, not unoccluded.

device=None: numpy.  device="cuda": the kernels, on device tensors.  The caller chooses; neither falls back to the other (the
convention of utils/normals.py and scene/strand_export.py)."""
import collections

import numpy as np

from data import capture
from data.colmap import qvec2rotmat

MAX_VIEWS = 4096
PINHOLES = ("SIMPLE_PINHOLE", "PINHOLE")

View = collections.namedtuple("View", ["R", "t", "fx", "fy", "cx", "cy", "W", "H", "name"])


def view_of(camera, image):
    """The View of a data.colmap Camera and Image."""
    if camera.model not in PINHOLES:
        raise ValueError(f"camera {camera.id} is a {camera.model} camera: the carving takes PINHOLE and SIMPLE_PINHOLE views only "
                         "(undistort.py turns a distorted capture into one of pinholes)")
    p = [float(v) for v in np.asarray(camera.params, np.float64).reshape(-1)]
    fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if camera.model == "SIMPLE_PINHOLE" else (p[0], p[1], p[2], p[3])
    return View(R=np.asarray(qvec2rotmat(np.asarray(image.qvec, np.float64)), np.float64), t=np.asarray(image.tvec, np.float64).reshape(3),
                fx=fx, fy=fy, cx=cx, cy=cy, W=int(camera.width), H=int(camera.height), name=image.name)


def check_count(n):
    if not 1 <= n <= MAX_VIEWS:
        raise ValueError(f"{n} views (1 to {MAX_VIEWS})")


def load_views(sparse_dir):
    """The Views of a sparse model (binary or text), in its images' order; ValueError for a camera that is no pinhole or a view count
    out of range."""
    cameras, images = capture.read_sparse(sparse_dir)
    views = [view_of(cameras[im.camera_id], im) for im in images.values()]
    check_count(len(views))
    return views


def read_plane(path, view, what, mode="L", sized=None):
    """The uint8 plane of a view read by data.capture.read_image (any format) and converted to `mode` ([H, W] for L, as the loader
    reads a mask; [H, W, 3] for RGB), writable.  ValueError for a missing file, which `what` names ("the mask"), or a size that is not
    the camera's (`sized`, by default `what`)."""
    a, _ = capture.read_image(path, (view.W, view.H), sized or what, "its camera", convert=mode, formats=None,
                              of=f"{what} of view {view.name}")
    return np.array(a)                                           # (a writable copy: PIL hands out a read-only view)


def check_views(views, masks, images=None):
    check_count(len(views))
    if len(masks) != len(views) or (images is not None and len(images) != len(views)):
        raise ValueError("one mask (and one image) per view")
    for k, v in enumerate(views):
        if masks[k].dtype != np.uint8 or masks[k].shape != (v.H, v.W):
            raise ValueError(f"view {k} ({v.name}): a uint8 mask of {v.W} x {v.H} pixels expected, got {masks[k].dtype} {masks[k].shape}")
        if images is not None and (images[k].dtype != np.uint8 or images[k].shape != (v.H, v.W, 3)):
            raise ValueError(f"view {k} ({v.name}): a uint8 image [{v.H}, {v.W}, 3] expected, got {images[k].dtype} {images[k].shape}")


def check_planes(views, planes, what):
    """One more uint8 plane [H, W] per view (`what` names it)."""
    if len(planes) != len(views):
        raise ValueError(f"one {what} plane per view")
    for k, v in enumerate(views):
        if planes[k].dtype != np.uint8 or planes[k].shape != (v.H, v.W):
            raise ValueError(f"view {k} ({v.name}): a uint8 {what} plane of {v.W} x {v.H} pixels expected, got {planes[k].dtype} "
                             f"{planes[k].shape}")


def is_cuda(device):
    if device is None:
        return False
    if not str(device).startswith("cuda"):
        raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernels)")
    return True


# ---- numpy path ------------------------------------------------------------------------------------------------------
def camera(view, x, y, z):
    """(xc, yc, zc) of float64 arrays."""
    R, t = view.R, view.t
    with np.errstate(all="ignore"):
        xc = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
        yc = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
        zc = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
    return xc, yc, zc


def image_point(view, xc, yc, zc):
    """(u, v) of camera coordinates."""
    with np.errstate(all="ignore"):
        return view.fx * (xc / zc) + view.cx, view.fy * (yc / zc) + view.cy


def pixel(view, xc, yc, zc):
    """(seen, py, px) of camera coordinates; py, px are 0 where not seen."""
    u, v = image_point(view, xc, yc, zc)
    with np.errstate(all="ignore"):
        seen = (zc > 0.0) & (u >= 0.0) & (u < view.W) & (v >= 0.0) & (v < view.H)
    px = np.floor(np.where(seen, u, 0.0)).astype(np.int64)
    py = np.floor(np.where(seen, v, 0.0)).astype(np.int64)
    return seen, py, px


# ---- device path -----------------------------------------------------------------------------------------------------
def upload_planes(planes, device):
    """The arrays of one dtype flattened, one after another, into one device buffer."""
    import torch
    return torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).to(device)


def upload_points(points, device):
    """A float64 device tensor [N, 3] of a host array."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))).to(device)


class Packed:
    """The views of a capture on the device: records (the host copy, an hgs_runtime.CarveView array), views_dev (its bytes), masks_dev
    and images_dev (or None): every mask / image flattened into one uint8 buffer, at the records' offsets."""

    def __init__(self, records, views_dev, masks_dev, images_dev=None):
        self.records, self.views_dev, self.masks_dev, self.images_dev = records, views_dev, masks_dev, images_dev


def pack(views, masks, images=None, device="cuda"):
    import ctypes
    import torch
    import hgs_runtime as rt
    check_views(views, masks, images)
    records = (rt.CarveView * len(views))()
    mask_offset = image_offset = 0
    for k, v in enumerate(views):
        r = records[k]
        r.R[:] = [float(a) for a in np.asarray(v.R, np.float64).reshape(9)]
        r.t[:] = [float(a) for a in np.asarray(v.t, np.float64).reshape(3)]
        r.fx, r.fy, r.cx, r.cy, r.W, r.H = float(v.fx), float(v.fy), float(v.cx), float(v.cy), v.W, v.H
        r.mask_offset, r.image_offset = mask_offset, image_offset if images is not None else -1
        mask_offset += v.W * v.H
        image_offset += 3 * v.W * v.H
    raw = np.frombuffer(ctypes.string_at(ctypes.addressof(records), ctypes.sizeof(records)), np.uint8).copy()
    images_dev = upload_planes(images, device) if images is not None else None
    return Packed(records, torch.from_numpy(raw).to(device), upload_planes(masks, device), images_dev)
