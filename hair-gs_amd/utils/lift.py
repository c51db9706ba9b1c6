"""3-D hair directions lifted from a capture's 2-D orientation maps: every point of the Stage-I cloud gets the line that its image
lines in the calibrated views agree on (the classical line-based multi-view step of hair capture; init_cloud.py --directions is the
driver, scene/gaussian_model.py direction_init the consumer; the reference starts Stage I from isotropic Gaussians).

The contract (this module's numpy path, csrc/hgs_lift.hip and the tests' loop restatement state the same thing).  All arithmetic is
float64 with one rounding per operation, in exactly the order written (the kernel file is built with -ffp-contract=off).

Inputs per view k.  The View of utils/views.py and three uint8 planes [H, W]: mask, orient and conf.  theta = orient*pi/255 and
confidence = conf/255 (the loader's rule, data/dataset_readers.py).  The map's angle is the one the orientation loss compares
against: theta = atan2(x, y) of the view-space direction, in [0, pi), measured from the image y axis, so the image line direction in
pixel units is l = (lu, lv) = (sin theta, cos theta).  sin and cos come from a table TAB[256][2] = (sin, cos)(o*pi/255), built once
on the host in float64 (table()) and handed to both backends: no transcendental is evaluated on the device.

Sample of a point (x, y, z) in view k.  xc, yc, zc, u, v, seen, px, py by utils/views.py's projection contract:
    used  iff  seen  and  mask[py, px] != 0  and  conf[py, px] >= min_conf       (min_conf: an integer, 0 to 255, default 1)
With visible (utils/visibility.py's words, int32 [N, ceil(V/32)]; None: no gate) a view is used only where, in addition, bit k % 32
of visible[i, k // 32] is set.  A point left with fewer than min_views used views gets the zero direction like any other such point:
there is no fallback to the ungated fit.  With every bit set the results are those without the gate, bit for bit.

The plane through the camera centre that contains the point's ray and the image line, with o = orient[py, px]:
    lu = TAB[o][0], lv = TAB[o][1];   a = lu/fx,  b = lv/fy
    ncx = -(zc*b),  ncy = zc*a,  ncz = xc*b - yc*a                       (its normal in the camera frame)
    n_i = (R0i*ncx + R1i*ncy) + R2i*ncz,  i = 0, 1, 2                    (world frame: R^T nc)
    nn  = (n0*n0 + n1*n1) + n2*n2
The view is skipped, and is not `used`, when nn is not > 0 or is not finite.  No square root is taken in this stage.

The weight.  w = conf[py, px]/255.0.  With a previous direction p (see Rounds) that is not the zero vector:
    r2 = ((n0*p0 + n1*p1) + n2*p2)^2 / nn        (the square is formed first, then divided)
    w  = w * (s2 / (s2 + r2))                    (s2 = sin(sigma)^2, computed once on the host)
A point whose p is (0, 0, 0) takes the plain weight.

The moments.  Views are visited in index order; for a used view, with g = w/nn:
    M += g * (n0*n0, n0*n1, n0*n2, n1*n1, n1*n2, n2*n2)      (each product is formed first, then multiplied by g, then added)
    wsum += w,  count += 1
lift_moments(...) returns M f64 [N, 6], wsum f64 [N] and count i32 [N].  The two backends agree on them bit for bit: the sums have
this fixed order, not an arbitrary one.

The solve.  lift_solve(M, count, min_views) returns d f64 [N, 3] and coherence f64 [N].  With the eigenvalues l0 <= l1 <= l2 of the
symmetric matrix: d is the unit eigenvector of l0, signed so that its component of largest magnitude is positive (lowest index on a
tie); coherence = (l1 - l0)/(l1 + l0), and 0 where the denominator is not > 0.  d = 0 and coherence = 0 where count < min_views
(default 2, minimum 2), where l1 <= 0 (a rank below 2 leaves the line undetermined) or where an entry of M is not finite.  Host:
numpy.linalg.eigh; device: cyclic Jacobi.  The two solvers agree to a tolerance (tests/test_lift_gpu.py), not to the bit.

Rounds.  lift_directions(...) is a host loop: round 0 has no previous direction, round r passes the d of round r - 1, and `rounds`
re-weighted rounds follow round 0 (rounds = 0 is the plain least-squares fit).  It returns (d, coherence, count) of the last round.
rounds = 3 and sigma = 10 degrees are knobs, not measured optima: a numpy prototype gave, at 16 ring views with half of the views
given a random angle, a median error of 14 degrees after round 0, 2.9 after three re-weighted rounds and 2.6 after four.

Known limits.  Without the gate "used" means in frame, on the mask and confident, not unoccluded: a far-side view contributes the
orientation of whatever hair it sees at that pixel, and the re-weighting is the only defence against that.  The gate is the other
one: utils/visibility.py marches the carved hull from the point to every camera, and init_cloud.py --directions --visibility hands
its words to the lift.  A direction along the common viewing axis of all its views is poorly determined.

device=None: numpy.  device="cuda": the kernels, on device tensors.  The caller chooses; neither falls back to the other."""
import math

import numpy as np

from utils.views import camera, check_planes, check_views, is_cuda, pack as pack_views, pixel, upload_planes, upload_points
from utils.visibility import check_words, view_bit


def table():
    """TAB f64 [256, 2]: (sin, cos) of o*pi/255."""
    theta = np.arange(256) * np.pi / 255
    return np.ascontiguousarray(np.stack([np.sin(theta), np.cos(theta)], axis=1))


def sin2(sigma_deg):
    s2 = math.sin(math.radians(float(sigma_deg))) ** 2
    if not (math.isfinite(s2) and s2 > 0.0):
        raise ValueError(f"sigma_deg = {sigma_deg}: sin(sigma)^2 must be finite and positive")
    return s2


def _check_planes(views, masks, orients, confs):
    check_views(views, masks)
    check_planes(views, orients, "orientation")
    check_planes(views, confs, "confidence")


def _check_knobs(min_conf=1, min_views=2):
    if int(min_conf) != min_conf or not 0 <= min_conf <= 255 or int(min_views) != min_views or min_views < 2:
        raise ValueError(f"min_conf = {min_conf} (an integer, 0 to 255), min_views = {min_views} (an integer >= 2)")
    return int(min_conf), int(min_views)


def _check_prev(prev, N):
    if prev is None:
        return None
    prev = np.asarray(prev, np.float64)
    if prev.shape != (N, 3):
        raise ValueError(f"prev of shape {prev.shape}: [{N}, 3] expected")
    return prev


# ---- numpy path ------------------------------------------------------------------------------------------------------
def _accumulate(acc, view, cam, used, o, c, tab, prev, s2):
    """One view's term of the moments; acc = (M, wsum, count), updated in place."""
    M, wsum, count = acc
    xc, yc, zc = cam
    R = view.R
    a, b = tab[o, 0] / view.fx, tab[o, 1] / view.fy
    ncx, ncy, ncz = -(zc * b), zc * a, xc * b - yc * a
    n = [(R[0, i] * ncx + R[1, i] * ncy) + R[2, i] * ncz for i in range(3)]
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    used = used & (nn > 0.0) & np.isfinite(nn)
    w = c / 255.0
    if prev is not None:
        dot = (n[0] * prev[:, 0] + n[1] * prev[:, 1]) + n[2] * prev[:, 2]
        r2 = (dot * dot) / nn
        plain = (prev[:, 0] == 0.0) & (prev[:, 1] == 0.0) & (prev[:, 2] == 0.0)
        w = np.where(plain, w, w * (s2 / (s2 + r2)))
    g = w / nn
    for j, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        M[:, j] = np.where(used, M[:, j] + g * (n[p] * n[q]), M[:, j])
    wsum[:] = np.where(used, wsum + w, wsum)
    count += used


def _moments_loop(points, views, prev, s2, sample, visible=None):
    points = np.asarray(points, np.float64).reshape(-1, 3)
    N = points.shape[0]
    prev = _check_prev(prev, N)
    if visible is not None:
        visible = check_words(visible, N, len(views))
    if prev is not None and not (math.isfinite(s2) and s2 > 0.0):
        raise ValueError(f"s2 = {s2}: finite and positive expected with a previous direction")
    tab = table()
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    acc = (np.zeros((N, 6), np.float64), np.zeros(N, np.float64), np.zeros(N, np.int32))
    with np.errstate(all="ignore"):
        for k, view in enumerate(views):
            cam = camera(view, x, y, z)
            used, o, c = sample(k, view, cam)
            if visible is not None:
                used = used & view_bit(visible, k)
            _accumulate(acc, view, cam, used, o.astype(np.int64), c.astype(np.float64), tab, prev, s2)
    return acc


def moments_numpy(points, views, masks, orients, confs, prev=None, s2=0.0, min_conf=1, visible=None):
    _check_planes(views, masks, orients, confs)
    min_conf, _ = _check_knobs(min_conf)

    def sample(k, view, cam):
        seen, py, px = pixel(view, *cam)
        c = confs[k][py, px]
        return seen & (masks[k][py, px] != 0) & (c >= min_conf), orients[k][py, px], c
    return _moments_loop(points, views, prev, s2, sample, visible)


def moments_from_samples(points, views, used, orient, conf, prev=None, s2=0.0, visible=None):
    """The moments without planes: used bool [V, N], orient and conf uint8 [V, N] give every (view, point) its sample directly (a point
    out of a view's frame is still not used)."""
    used, orient, conf = np.asarray(used, bool), np.asarray(orient, np.uint8), np.asarray(conf, np.uint8)

    def sample(k, view, cam):
        return used[k] & pixel(view, *cam)[0], orient[k], conf[k]
    return _moments_loop(points, views, prev, s2, sample, visible)


def symmetric(M):
    """[N, 6] (00, 01, 02, 11, 12, 22) -> [N, 3, 3]."""
    M = np.asarray(M, np.float64).reshape(-1, 6)
    return M[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def solve_numpy(M, count, min_views=2):
    _, min_views = _check_knobs(1, min_views)
    M, count = np.asarray(M, np.float64).reshape(-1, 6), np.asarray(count).reshape(-1)
    N = M.shape[0]
    d, coherence = np.zeros((N, 3), np.float64), np.zeros(N, np.float64)
    ok = np.isfinite(M).all(axis=1) & (count >= min_views)
    if not ok.any():
        return d, coherence
    lam, vec = np.linalg.eigh(symmetric(M[ok]))
    v = vec[:, :, 0]
    top = np.argmax(np.abs(v), axis=1)                           # (the first index on a tie)
    v = np.where(v[np.arange(v.shape[0]), top][:, None] < 0.0, -v, v)
    den = lam[:, 1] + lam[:, 0]
    with np.errstate(all="ignore"):
        coh = np.where(den > 0.0, (lam[:, 1] - lam[:, 0]) / den, 0.0)
    line = lam[:, 1] > 0.0
    d[ok] = np.where(line[:, None], v, 0.0)
    coherence[ok] = np.where(line, coh, 0.0)
    return d, coherence


# ---- device path -----------------------------------------------------------------------------------------------------
class Packed:
    """A capture's views on the device for the lift: carve (a utils.views.Packed: records, views_dev, masks_dev), orients_dev and
    confs_dev (laid out like masks_dev, at the records' mask_offset) and tab_dev (TAB, float64 [256, 2])."""

    def __init__(self, carve, orients_dev, confs_dev, tab_dev):
        self.carve, self.orients_dev, self.confs_dev, self.tab_dev = carve, orients_dev, confs_dev, tab_dev


def pack(views, masks, orients, confs, device="cuda", carve_packed=None):
    """carve_packed: the same views and masks already packed by utils.views.pack (the driver's), reused as they are."""
    import torch
    _check_planes(views, masks, orients, confs)
    if carve_packed is None:
        carve_packed = pack_views(views, masks, None, device)
    return Packed(carve_packed, upload_planes(orients, device), upload_planes(confs, device), torch.from_numpy(table()).to(device))


def moments_device(points, packed, prev=None, s2=0.0, min_conf=1, visible=None):
    """hgs_lift_moments on a float64 device tensor [N, 3]: (M [N, 6] f64, wsum [N] f64, count [N] i32) on its device.  With visible
    (an int32 device tensor [N, ceil(V/32)]): hgs_lift_moments_gated."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(points, "points", torch.float64)
    if points.dim() != 2 or points.shape[1] != 3:
        raise rt.HgsError(f"points of shape {tuple(points.shape)}: [N, 3] expected")
    N = points.shape[0]
    if prev is not None:
        rt.require_device_buffer(prev, "prev", torch.float64)
        if tuple(prev.shape) != (N, 3):
            raise rt.HgsError(f"prev of shape {tuple(prev.shape)}: [{N}, 3] expected")
    V = rt.lift_check(packed.carve.records, packed.carve.views_dev, packed.carve.masks_dev, packed.orients_dev, packed.confs_dev,
                      packed.tab_dev, packed.carve.images_dev, visible, N)
    M = torch.empty((N, 6), dtype=torch.float64, device=points.device)
    wsum = torch.empty(N, dtype=torch.float64, device=points.device)
    count = torch.empty(N, dtype=torch.int32, device=points.device)
    head = (rt.current_stream(), N, rt.ptr(points), V, rt.ptr(packed.carve.views_dev), rt.ptr(packed.carve.masks_dev),
            rt.ptr(packed.orients_dev), rt.ptr(packed.confs_dev), rt.ptr(packed.tab_dev), rt.ptr(prev),
            float(s2) if prev is not None else 0.0, int(min_conf))
    tail = (rt.ptr(M), rt.ptr(wsum), rt.ptr(count))
    with torch.cuda.device(points.device):
        if visible is None:
            rt.check(rt.lib().hgs_lift_moments(*head, *tail))
        else:
            rt.check(rt.lib().hgs_lift_moments_gated(*head, rt.ptr(visible), visible.shape[1], *tail))
    return M, wsum, count


def solve_device(M, count, min_views=2):
    """hgs_lift_solve: (d [N, 3] f64, coherence [N] f64) on the device of M."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(M, "M", torch.float64)
    rt.require_device_buffer(count, "count", torch.int32)
    if M.dim() != 2 or M.shape[1] != 6 or tuple(count.shape) != (M.shape[0],):
        raise rt.HgsError(f"M of shape {tuple(M.shape)} with count of shape {tuple(count.shape)}: [N, 6] and [N] expected")
    N = M.shape[0]
    d = torch.empty((N, 3), dtype=torch.float64, device=M.device)
    coherence = torch.empty(N, dtype=torch.float64, device=M.device)
    with torch.cuda.device(M.device):
        rt.check(rt.lib().hgs_lift_solve(rt.current_stream(), N, rt.ptr(M), rt.ptr(count), int(min_views), rt.ptr(d), rt.ptr(coherence)))
    return d, coherence


def directions_device(points, packed, rounds=3, sigma_deg=10.0, min_conf=1, min_views=2, visible=None):
    """The rounds on device tensors: (d, coherence, count)."""
    s2 = sin2(sigma_deg)
    prev = None
    for _ in range(_check_rounds(rounds) + 1):
        M, _, count = moments_device(points, packed, prev, s2, min_conf, visible)
        prev, coherence = solve_device(M, count, min_views)
    return prev, coherence, count


# ---- host-array entry points -----------------------------------------------------------------------------------------
def _check_rounds(rounds):
    if int(rounds) != rounds or rounds < 0:
        raise ValueError(f"rounds = {rounds}: an integer >= 0")
    return int(rounds)


def _upload_words(visible, device):
    """The visibility words (a host int32 array [N, W], or None) as a device tensor."""
    if visible is None:
        return None
    import torch
    return torch.from_numpy(np.ascontiguousarray(visible)).to(device)


def lift_moments(points, views, masks, orients, confs, prev=None, s2=0.0, min_conf=1, device=None, visible=None):
    """(M f64 [N, 6], wsum f64 [N], count i32 [N]); host arrays.  visible: utils/visibility.py's words, int32 [N, ceil(V/32)]."""
    if not is_cuda(device):
        return moments_numpy(points, views, masks, orients, confs, prev, s2, min_conf, visible)
    pts = upload_points(points, device)
    out = moments_device(pts, pack(views, masks, orients, confs, device), None if prev is None else upload_points(prev, device), s2,
                         min_conf, _upload_words(visible, device))
    return tuple(t.cpu().numpy() for t in out)


def lift_solve(M, count, min_views=2, device=None):
    """(d f64 [N, 3], coherence f64 [N]); host arrays."""
    if not is_cuda(device):
        return solve_numpy(M, count, min_views)
    import torch
    M = torch.from_numpy(np.ascontiguousarray(np.asarray(M, np.float64).reshape(-1, 6))).to(device)
    count = torch.from_numpy(np.ascontiguousarray(np.asarray(count, np.int32).reshape(-1))).to(device)
    return tuple(t.cpu().numpy() for t in solve_device(M, count, min_views))


def lift_directions(points, views, masks, orients, confs, rounds=3, sigma_deg=10.0, min_conf=1, min_views=2, device=None, visible=None):
    """(d f64 [N, 3], coherence f64 [N], count i32 [N]) of the last round; host arrays."""
    rounds = _check_rounds(rounds)
    if is_cuda(device):
        out = directions_device(upload_points(points, device), pack(views, masks, orients, confs, device), rounds, sigma_deg, min_conf,
                                min_views, _upload_words(visible, device))
        return tuple(t.cpu().numpy() for t in out)
    s2 = sin2(sigma_deg)
    prev = None
    for _ in range(rounds + 1):
        M, _, count = moments_numpy(points, views, masks, orients, confs, prev, s2, min_conf, visible)
        prev, coherence = solve_numpy(M, count, min_views)
    return prev, coherence, count
