"""Which views can see a point of the carved hull: a ray from the point to every camera centre is marched through the occupancy grid
that utils/carve.py has just carved, and a view whose ray meets occupied voxels on the way is blocked.  The hair in front of a
far-side view is inside the hull by construction, so the grid already says which views look at other hair; utils/lift.py takes the
answer as its `visible` gate and init_cloud.py --directions --visibility is the driver.  The reference has no such step.

The contract (this module's numpy path, csrc/hgs_visibility.hip and the loop restatement in tests/visibility_reference.py state the
same thing).  All arithmetic is float64 with one rounding per operation, in exactly the order written (the kernel file is built with
-ffp-contract=off).

Inputs.  points f64 [N, 3]; centres f64 [V, 3], the camera centres -R^T t computed once on the host (camera_centres; a centre that
is not finite is refused), 1 <= V <= 4096; occ uint8 [nz, ny, nx] with origin f64 [3] and h, the carve's grid: voxel i spans
origin + i*h .. origin + (i + 1)*h per axis, 1 to 1024 voxels an axis (utils.carve's rule), h and 1/h finite and positive; integers
0 <= skip <= 1024 (default 1) and 0 <= max_blocked <= 3072 (default 0).

Output.  words int32 [N, ceil(V/32)]: bit k % 32 of word k // 32 is set iff view k is not blocked; the bits at and above V are 0.

Start of a ray, per axis a:  t_a = (p_a - origin_a)/h.  The start is inside iff 0 <= t_a < n_a on every axis (a NaN fails the
comparison, which comes before any conversion to an integer).  A point that does not start inside has every bit below V set: it is
unoccluded, which is the lift's behaviour without a gate.  Otherwise i0_a = (int)floor(t_a).

Ray setup, with D = C - p, per axis:
    D_a > 0:   step = +1,  tmax = ((origin_a + (i0_a + 1)*h) - p_a)/D_a,  td = h/D_a
    D_a < 0:   step = -1,  tmax = ((origin_a + i0_a*h) - p_a)/D_a,        td = h/(-D_a)
    D_a == 0:  step = 0,   tmax = +inf
Walk, from i = i0 with blocked = 0:
    1. a = the axis of the smallest tmax, compared with strict < (x, then y, then z: the lowest axis wins a tie)
    2. stop VISIBLE unless tmax_a < 1.0                                   (the camera has been reached)
    3. i_a = i_a + step_a;  stop VISIBLE if i_a has left the grid
    4. tmax_a = tmax_a + td_a
    5. if max_a |i_a - i0_a| > skip and occ[i] != 0:  blocked = blocked + 1;  stop BLOCKED if blocked > max_blocked
    6. at most nx + ny + nz steps, then VISIBLE
The indices move monotonically and stay inside the grid between steps, so a ray takes at most (nx - 1) + (ny - 1) + (nz - 1) steps
inside and one that leaves: the cap of step 6 cannot be reached, and stands only so that the loop is bounded on its face.  The start
voxel is never tested (its distance 0 is not > skip), and neither is anything beyond the camera.

Known limits.  Visibility is only as good as the hull: a loose hull hides nothing it should not, but a hole in a mask lets a ray
through.  Grazing views, whose ray runs along the surface through occupied voxels, are dropped.  skip is in voxels and is a knob:
with 0 a shell point's own neighbours on the surface block views that do see it, with a large one nearby hair no longer blocks.
The hull points' colours are still averaged over all hits (init_cloud.py).

device=None: numpy (vectorised over the (point, view) pairs that are still walking, as utils/trace.py's tracer is over its strands).
device="cuda": the kernel, on device tensors.  The caller chooses; neither falls back to the other."""
import math

import numpy as np

from utils.carve import _check_grid
from utils.views import MAX_VIEWS, camera, is_cuda, pixel, upload_points

MAX_SKIP, MAX_BLOCKED = 1024, 3072
_PAIRS = 1 << 21                  # (point, view) pairs per numpy pass of the march


def camera_centres(views):
    """C f64 [V, 3] = -R^T t of the views; ValueError for a centre that is not finite."""
    C = np.stack([-(np.asarray(v.R, np.float64).T @ np.asarray(v.t, np.float64).reshape(3)) for v in views]) if len(views) else np.zeros((0, 3))
    return _check_centres(C)


def _check_centres(centres, error=ValueError):
    C = np.ascontiguousarray(np.asarray(centres, np.float64))
    if C.ndim != 2 or C.shape[1] != 3 or not 1 <= C.shape[0] <= MAX_VIEWS:
        raise error(f"centres of shape {C.shape}: [V, 3] with 1 to {MAX_VIEWS} views expected")
    if not np.isfinite(C).all():
        raise error(f"the centre of view {int(np.flatnonzero(~np.isfinite(C).all(axis=1))[0])} is not finite")
    return C


def check_knobs(skip=1, max_blocked=0, error=ValueError):
    if int(skip) != skip or int(max_blocked) != max_blocked or not 0 <= skip <= MAX_SKIP or not 0 <= max_blocked <= MAX_BLOCKED:
        raise error(f"skip = {skip} (an integer, 0 to {MAX_SKIP}), max_blocked = {max_blocked} (an integer, 0 to {MAX_BLOCKED})")
    return int(skip), int(max_blocked)


def check_grid(origin, h, dims, error=ValueError):
    """(origin f64 [3], h, (nx, ny, nz)) of a grid the contract allows."""
    h = float(h)
    dims = _check_grid(h, dims, error)
    origin = np.asarray(origin, np.float64).reshape(-1)
    if origin.shape != (3,) or not np.isfinite(origin).all() or not (math.isfinite(1.0 / h) and 1.0 / h > 0.0):
        raise error(f"origin {origin.tolist()} and voxel size {h}: finite, the size and 1/size > 0")
    return np.ascontiguousarray(origin), h, dims


def word_count(V):
    return (int(V) + 31) // 32


def all_visible(N, V):
    """The words of N points that every one of V views sees."""
    bits = np.arange(word_count(V) * 32).reshape(-1, 32) < V
    row = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32).view(np.int32)
    return np.repeat(row[None, :], int(N), axis=0)


def pack_bits(visible):
    """bool [N, V] -> words int32 [N, ceil(V/32)]."""
    visible = np.asarray(visible, bool)
    N, V = visible.shape
    bits = np.zeros((N, word_count(V) * 32), np.uint64)
    bits[:, :V] = visible
    return np.ascontiguousarray((bits.reshape(N, word_count(V), 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32).view(np.int32))


def view_bit(words, k):
    """bool [N]: bit k of the words int32 [N, W]."""
    return ((np.asarray(words)[:, k // 32] >> (k % 32)) & 1) != 0


def unpack_bits(words, V):
    """words int32 [N, ceil(V/32)] -> bool [N, V]."""
    words = check_words(words, np.asarray(words).shape[0], V)
    return np.stack([view_bit(words, k) for k in range(V)], axis=1) if V else np.zeros((words.shape[0], 0), bool)


def check_words(words, N, V, error=ValueError):
    words = np.asarray(words)
    if words.dtype != np.int32 or words.shape != (N, word_count(V)):
        raise error(f"visible of dtype {words.dtype} and shape {words.shape}: int32 [{N}, {word_count(V)}] expected")
    return words


# ---- numpy path ------------------------------------------------------------------------------------------------------
def _march(p, i0, C, occ, origin, h, dims, skip, max_blocked):
    """blocked bool [n, V] of n points that start inside (i0 int64 [n, 3])."""
    n, V = p.shape[0], C.shape[0]
    nx, ny, nz = dims
    top = np.array(dims, np.int64)
    with np.errstate(all="ignore"):
        P = np.repeat(p, V, axis=0)                              # [n*V, 3]: pair j is (point j // V, view j % V)
        I0 = np.repeat(i0, V, axis=0)
        D = np.tile(C, (n, 1)) - P
        pos, neg = D > 0.0, D < 0.0
        edge = np.where(pos, origin + (I0 + 1).astype(np.float64) * h, origin + I0.astype(np.float64) * h)
        tmax = np.where(pos | neg, (edge - P) / D, np.inf)
        td = np.where(pos, h / D, h / (-D))
    step = pos.astype(np.int64) - neg.astype(np.int64)
    idx = I0.copy()
    count = np.zeros(n * V, np.int64)
    blocked = np.zeros(n * V, bool)
    alive = np.arange(n * V)
    for _ in range(nx + ny + nz):
        if alive.size == 0:
            break
        t = tmax[alive]
        a = np.where(t[:, 1] < t[:, 0], 1, 0)
        a = np.where(t[:, 2] < t[np.arange(alive.size), a], 2, a)
        go = t[np.arange(alive.size), a] < 1.0
        alive, a = alive[go], a[go]
        idx[alive, a] += step[alive, a]
        go = (idx[alive, a] >= 0) & (idx[alive, a] < top[a])
        alive, a = alive[go], a[go]
        tmax[alive, a] = tmax[alive, a] + td[alive, a]
        i = idx[alive]
        hit = (np.abs(i - I0[alive]).max(axis=1) > skip) & (occ[i[:, 2], i[:, 1], i[:, 0]] != 0)
        count[alive] += hit
        stop = count[alive] > max_blocked
        blocked[alive[stop]] = True
        alive = alive[~stop]
    return blocked.reshape(n, V)


def visibility_numpy(points, centres, occ, origin, h, skip=1, max_blocked=0):
    points = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    C = _check_centres(centres)
    occ = np.asarray(occ)
    if occ.ndim != 3 or occ.dtype != np.uint8:
        raise ValueError("occ must be uint8 [nz, ny, nx]")
    origin, h, dims = check_grid(origin, h, occ.shape[::-1])
    skip, max_blocked = check_knobs(skip, max_blocked)
    N, V = points.shape[0], C.shape[0]
    words = all_visible(N, V)
    with np.errstate(all="ignore"):
        t = (points - origin) / h
        inside = ((t >= 0.0) & (t < np.array(dims, np.float64))).all(axis=1)
    rows = np.flatnonzero(inside)
    i0 = np.floor(t[rows]).astype(np.int64)
    per = max(1, _PAIRS // V)
    for s in range(0, rows.size, per):
        r = rows[s:s + per]
        words[r] = pack_bits(~_march(points[r], i0[s:s + per], C, occ, origin, h, dims, skip, max_blocked))
    return words


# ---- device path -----------------------------------------------------------------------------------------------------
def visibility_device(points, centres, occ, origin, h, skip=1, max_blocked=0):
    """hgs_hull_visibility on device tensors (points f64 [N, 3], centres f64 [V, 3], occ uint8 [nz, ny, nx]): the words, an int32
    tensor [N, ceil(V/32)] on their device."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(occ, "occ", torch.uint8)
    if occ.dim() != 3:
        raise rt.HgsError("occ must be uint8 [nz, ny, nx]")
    nz, ny, nx = occ.shape
    origin, h, _ = check_grid(origin, h, (nx, ny, nz), error=rt.HgsError)
    skip, max_blocked = check_knobs(skip, max_blocked, error=rt.HgsError)
    rt.require_device_buffer(points, "points", torch.float64)
    if points.dim() != 2 or points.shape[1] != 3:
        raise rt.HgsError(f"points of shape {tuple(points.shape)}: [N, 3] expected")
    N = points.shape[0]
    rt.require_device_buffer(centres, "centres", torch.float64)
    if centres.dim() != 2 or centres.shape[1] != 3 or not 1 <= centres.shape[0] <= MAX_VIEWS:
        raise rt.HgsError(f"centres of shape {tuple(centres.shape)}: [V, 3] with 1 to {MAX_VIEWS} views expected")
    V = centres.shape[0]
    words = torch.empty((N, word_count(V)), dtype=torch.int32, device=points.device)
    rt.visibility_check((nx, ny, nz), occ, points, centres, words)
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_hull_visibility(rt.current_stream(), N, rt.ptr(points), V, rt.ptr(centres), rt.ptr(occ), origin.ctypes.data, h,
                                              nx, ny, nz, skip, max_blocked, rt.ptr(words)))
    return words


def upload_centres(centres, device):
    """The checked centres as a float64 device tensor [V, 3]."""
    import hgs_runtime as rt
    return upload_points(_check_centres(centres, error=rt.HgsError), device)


# ---- host-array entry point ------------------------------------------------------------------------------------------
def hull_visibility(points, centres, occ, origin, h, skip=1, max_blocked=0, device=None):
    """words int32 [N, ceil(V/32)], a host array."""
    if not is_cuda(device):
        return visibility_numpy(points, centres, occ, origin, h, skip, max_blocked)
    import torch
    occ_dev = torch.from_numpy(np.ascontiguousarray(occ)).to(device)
    return visibility_device(upload_points(points, device), upload_centres(centres, device), occ_dev, origin, h, skip, max_blocked).cpu().numpy()


def pair_counts(points, views, masks, words):
    """(on_mask, visible) int64: the (point, view) pairs in frame and on the mask, and those of them whose bit is set.  Host
    arithmetic for the driver's report, not part of the contract."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    words = check_words(words, points.shape[0], len(views))
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    on_mask = visible = 0
    for k, view in enumerate(views):
        seen, py, px = pixel(view, *camera(view, x, y, z))
        hit = seen & (masks[k][py, px] != 0)
        on_mask += int(hit.sum())
        visible += int((hit & view_bit(words, k)).sum())
    return on_mask, visible
