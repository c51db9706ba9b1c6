"""Strands grown from the scalp through the lifted hair directions: the step that classically follows the line-based multi-view lift
of utils/lift.py.  init_cloud.py --directions gives every carved point a 3-D hair line, init_scalp.py the strand roots, head_sdf.py the
head's distance field; this module splats the lines into a direction volume and traces a polyline from every root through it.
trace_strands.py is the scene driver; the result is a strand model that train.py refines as Stage III and export_strands.py writes as
a hair asset.  The reference has no such step.

The contract (this module's numpy paths, csrc/hgs_trace.hip and the loop restatement in tests/trace_reference.py state the same
thing).  All arithmetic is float64 with one rounding per operation, in exactly the order written (the kernel file is built with
-ffp-contract=off).  dot(u, v) = (u0*v0 + u1*v1) + u2*v2 throughout.

Grid.  Node (ix, iy, iz) lies at p = origin + index*h per axis; 2 <= n_axis <= 1024 and at most 2^26 nodes in all (MAX_NODES: the
seven sums of that many nodes take 3.5 GiB, the field 2 GiB).  Arrays are laid out [nz, ny, nx, ...].

Splat.  points f64 [N, 3], dirs f64 [N, 3], N <= 2^24; r2 = r*r formed on the host, r <= 8 h.  A point whose coordinates are not
finite is skipped and counted; so is a point whose dot(dir, dir) is not finite or not > 0.  For the others d = dir / sqrt(dot(dir,
dir)) (three divisions) and, for every node p:
    dx = p - x per axis,  d2 = dot(dx, dx);  the point contributes  iff  d2 < r2;  k = 1 - d2/r2
    Wq    += rint(k * 4294967296.0)
    Tq_ab += rint((k * m) * 4294967296.0)   for the six products m = d_a*d_b (xx, xy, xz, yy, yz, zz)
rint is round-half-even.  The seven sums are int64, acc [nz, ny, nx, 7] = (W, xx, xy, xz, yy, yz, zz).  Integer sums are exact: they
do not depend on the order of the points, on how the cloud is split into calls or on the launch.  Both paths visit, per point, a box
of nodes that holds every node closer than r with 1/64 of a spacing to spare for the roundings of the node positions (good while
|origin| / h < 2^40); a point further than r outside the grid meets no node.  2^24 points of weight <= 2^32 cannot overflow.

Solve.  T = Tq * 2^-32 (W likewise).  With the eigenvalues l0 <= l1 <= l2 of T: dir is the unit eigenvector of l2 with its component
of largest magnitude positive (lowest index on a tie); conf = l2 - l1, the aligned mass in units of one fully weighted point.  dir = 0
and conf = 0 where Wq == 0 or an entry is not finite.  Host: numpy.linalg.eigh; device: cyclic Jacobi (csrc/hgs_jacobi3.h).  The two
agree to a tolerance (tests/test_trace_gpu.py), not to the bit.  dir f64 [nz, ny, nx, 3], conf f64 [nz, ny, nx].

Head exclusion.  Host arithmetic shared by both paths (exclude_head): a node whose utils.head_sdf.sample distance is < margin gets
conf = 0.

Trace.  roots f64 [S, 3], p0 f64 [S, 3] (unit initial directions), k = 1/h divided on the host, 1 <= max_steps <= 4096.  Per root:
x = root, p = p0, gap = 0, entered = false, n = 1, last = 0, joints[0] = root;
    repeat max_steps times:
      t = (x - origin)*k per axis;  unless every t is finite and 0 <= t < n_axis - 1:  stop BOUNDS
      i = floor(t), f = t - i;  g0 = 1 - f, g1 = f per axis
      w = 0, v = 0;  corners with z outermost, then y, then x, each 0 then 1:
         tw = (gx*gy)*gz;  a = tw*conf[corner];  w = w + a
         e = dir[corner];  if dot(e, p) < 0: a = -a
         v_j = v_j + a*e_j
      nn = dot(v, v)
      if w >= min_conf and nn is finite and > 0:
         d = v / sqrt(nn)
         if entered and dot(d, p) < cos_max:  stop TURN
         entered = true;  gap = 0
      else:
         gap = gap + 1;  if gap > max_gap:  stop GAP
         d = p
      x = x + step*d;  p = d;  joints[n] = x;  n = n + 1;  if gap == 0: last = n - 1
    stop STEPS
    count = last + 1
The turn test is off until the strand has taken its first field step: the approach from the scalp runs along the outward direction
and says nothing about hair, so on entry only the sign is chosen.  Coasted joints at the tail are cut (count).  joints f64 [S,
max_steps + 1, 3] (rows at and beyond count are unspecified), count i32 [S], reason i32 [S] (STEPS 0, BOUNDS 1, TURN 2, GAP 3).  The
range test precedes every load.  The kernel, trace_numpy (vectorised over the strands that are still alive) and the tests' loop give
equal bits on the same dir / conf; negating any dir entries changes no bit (a*e_j = (-a)*(-e_j)), dot(e, p) == 0 exactly aside.

Known limits.  Euler stepping drifts outward on curved hair (a prototype went from radius 0.6 to 0.97 over 150 half-voxel steps on a
circle of 5 voxels radius); a midpoint step is the obvious next knob.  Roots are never thinned by coverage.  The tracer does not push
a joint out of the head (train.py --lambda_head does).  A shell-only cloud yields outer-layer hair only.

device=None: numpy.  device="cuda": the kernels.  The caller chooses; neither falls back to the other (utils/carve.py's convention)."""
import math

import numpy as np

from utils.views import is_cuda

STEPS, BOUNDS, TURN, GAP = 0, 1, 2, 3
REASONS = ("steps", "bounds", "turn", "gap")
MAX_NODES, MAX_POINTS, MAX_ROOTS, MAX_STEPS, MAX_REACH = 1 << 26, 1 << 24, 1 << 24, 4096, 8.0
FIXED_ONE = 4294967296.0
BUDGET = 1 << 30                  # bytes of joints a batch of roots may take (trace)
FIELD_KEYS = ("origin", "spacing", "shape", "dir", "conf")
_PAIRS = 1 << 22                  # (point, box node) pairs per numpy pass of the splat


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _rows3(a, name):
    a = np.asarray(a, np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name} of shape {a.shape}: [N, 3] expected")
    return np.ascontiguousarray(a)


def check_grid(origin, h, shape):
    """(origin f64 [3], h, (nx, ny, nz)) of a grid the contract allows; ValueError otherwise."""
    origin = np.asarray(origin, np.float64).reshape(-1)
    h = float(h)
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or min(shape) < 2 or max(shape) > 1024 or shape[0] * shape[1] * shape[2] > MAX_NODES:
        raise ValueError(f"a grid of {shape} nodes (2 to 1024 an axis, at most 2^26 in all)")
    if origin.shape != (3,) or not (np.isfinite(origin).all() and math.isfinite(h) and h > 0.0 and math.isfinite(1.0 / h) and 1.0 / h > 0.0):
        raise ValueError(f"origin {origin.tolist()} and spacing {h}: finite, the spacing and 1/spacing > 0")
    return np.ascontiguousarray(origin), h, shape


def _check_radius(r, h):
    r = float(r)
    r2 = r * r
    if not (math.isfinite(r2) and r2 > 0.0 and math.sqrt(r2) / h <= MAX_REACH):
        raise ValueError(f"r = {r} with spacing {h}: r*r finite and > 0, r at most {MAX_REACH:g} spacings")
    return r2


class Field:
    """origin f64 [3], spacing, shape (nx, ny, nz), dir f64 [nz, ny, nx, 3], conf f64 [nz, ny, nx]."""

    def __init__(self, origin, spacing, shape, dir, conf):
        self.origin, self.spacing, self.shape = check_grid(origin, spacing, shape)
        nx, ny, nz = self.shape
        self.dir = np.ascontiguousarray(dir, dtype=np.float64)
        self.conf = np.ascontiguousarray(conf, dtype=np.float64)
        if self.dir.shape != (nz, ny, nx, 3) or self.conf.shape != (nz, ny, nx):
            raise ValueError(f"dir {self.dir.shape} and conf {self.conf.shape} for a grid of {self.shape} nodes: [nz, ny, nx, 3] and [nz, ny, nx]")

    def nodes(self):
        """f64 [nz*ny*nx, 3]: the node positions, origin + index*h."""
        nx, ny, nz = self.shape
        z, y, x = np.meshgrid(*(self.origin[a] + np.arange(n, dtype=np.float64) * self.spacing for a, n in ((2, nz), (1, ny), (0, nx))),
                              indexing="ij")
        return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


# ---- the direction volume: numpy path ------------------------------------------------------------------------------------
def _box(r2, h):
    reach = math.sqrt(r2) / h + 0.015625
    return reach, int(math.floor(2.0 * reach)) + 2


def splat_numpy(points, dirs, origin, h, shape, r, acc=None):
    """(acc int64 [nz, ny, nx, 7], skipped) of the contract's splat; `acc`, when given, is added to."""
    points, dirs = _rows3(points, "points"), _rows3(dirs, "dirs")
    origin, h, (nx, ny, nz) = check_grid(origin, h, shape)
    r2 = _check_radius(r, h)
    N = points.shape[0]
    if dirs.shape[0] != N or N > MAX_POINTS:
        raise ValueError(f"{N} points with {dirs.shape[0]} directions (equal counts, at most 2^24)")
    if acc is None:
        acc = np.zeros((nz, ny, nx, 7), np.int64)
    elif acc.shape != (nz, ny, nx, 7) or acc.dtype != np.int64 or not acc.flags.c_contiguous:
        raise ValueError(f"acc {acc.shape} {acc.dtype}: contiguous int64 [{nz}, {ny}, {nx}, 7] expected")
    flat = acc.reshape(-1, 7)
    reach, span = _box(r2, h)
    k = 1.0 / h
    n_axis = (nx, ny, nz)
    with np.errstate(all="ignore"):
        dd = _dot(dirs.T, dirs.T)
        good = np.isfinite(points).all(axis=1) & np.isfinite(dd) & (dd > 0.0)
        skipped = int(N - good.sum())
        pts = points[good]
        d = dirs[good] / np.sqrt(dd[good])[:, None]
        m = [d[:, a] * d[:, b] for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        start = [np.clip(np.floor((pts[:, a] - origin[a]) * k - reach), -span, n_axis[a]).astype(np.int64) for a in range(3)]
        rows = max(1, _PAIRS // span ** 3)
        off = np.arange(span, dtype=np.int64)
        for r0 in range(0, pts.shape[0], rows):
            sl = slice(r0, r0 + rows)
            idx = [start[a][sl, None] + off[None, :] for a in range(3)]                     # [n, span] per axis
            inside = [(idx[a] >= 0) & (idx[a] < n_axis[a]) for a in range(3)]
            e = [(origin[a] + idx[a].astype(np.float64) * h) - pts[sl, a, None] for a in range(3)]
            ex, ey, ez = e[0][:, None, None, :], e[1][:, None, :, None], e[2][:, :, None, None]   # [n, z, y, x]
            d2 = (ex * ex + ey * ey) + ez * ez
            hit = (d2 < r2) & inside[0][:, None, None, :] & inside[1][:, None, :, None] & inside[2][:, :, None, None]
            pi, zi, yi, xi = np.nonzero(hit)
            if pi.size == 0:
                continue
            w = 1.0 - d2[pi, zi, yi, xi] / r2
            node = (idx[2][pi, zi] * ny + idx[1][pi, yi]) * nx + idx[0][pi, xi]
            np.add.at(flat[:, 0], node, np.rint(w * FIXED_ONE).astype(np.int64))
            for j in range(6):
                np.add.at(flat[:, j + 1], node, np.rint((w * m[j][sl][pi]) * FIXED_ONE).astype(np.int64))
    return acc, skipped


def _t_matrices(acc):
    a = acc.reshape(-1, 7)
    T = a[:, 1:].astype(np.float64) * (1.0 / FIXED_ONE)
    return a[:, 0], T[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def solve_numpy(acc):
    """(dir f64 [..., 3], conf f64 [...]) of sums acc int64 [..., 7]."""
    acc = np.asarray(acc)
    if acc.dtype != np.int64 or acc.ndim < 1 or acc.shape[-1] != 7:
        raise ValueError(f"acc {acc.shape} {acc.dtype}: int64 [..., 7] expected")
    lead = acc.shape[:-1]
    Wq, T = _t_matrices(np.ascontiguousarray(acc))
    n = Wq.shape[0]
    d, conf = np.zeros((n, 3), np.float64), np.zeros(n, np.float64)
    ok = (Wq != 0) & np.isfinite(T).all(axis=(1, 2))
    if ok.any():
        lam, vec = np.linalg.eigh(T[ok])
        v = vec[:, :, 2]
        top = np.argmax(np.abs(v), axis=1)                       # (the first index on a tie)
        v = np.where(v[np.arange(v.shape[0]), top][:, None] < 0.0, -v, v)
        d[ok] = v
        conf[ok] = lam[:, 2] - lam[:, 1]
    return d.reshape(lead + (3,)), conf.reshape(lead)


# ---- the direction volume: device path -----------------------------------------------------------------------------------
def splat_device(points, dirs, origin, h, shape, r, acc=None, skipped=None):
    """hgs_field_splat on float64 device tensors [N, 3]: (acc int64 [nz, ny, nx, 7], skipped int32 [1]) on their device; both are
    added to when given (a cloud splatted in parts)."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(points, "points", torch.float64)
    rt.require_device_buffer(dirs, "dirs", torch.float64)
    if points.dim() != 2 or points.shape[1] != 3 or tuple(dirs.shape) != tuple(points.shape):
        raise rt.HgsError(f"points {tuple(points.shape)} and dirs {tuple(dirs.shape)}: [N, 3] both expected")
    try:
        origin, h, (nx, ny, nz) = check_grid(origin, h, shape)
        r2 = _check_radius(r, h)
    except ValueError as e:
        raise rt.HgsError(str(e)) from None
    if acc is None:
        acc = torch.zeros((nz, ny, nx, 7), dtype=torch.int64, device=points.device)
    if skipped is None:
        skipped = torch.zeros(1, dtype=torch.int32, device=points.device)
    rt.trace_check(acc, (nx, ny, nz), skipped=skipped)
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_field_splat(rt.current_stream(), points.shape[0], rt.ptr(points), rt.ptr(dirs), float(origin[0]),
                                          float(origin[1]), float(origin[2]), h, nx, ny, nz, r2, rt.ptr(acc), rt.ptr(skipped)))
    return acc, skipped


def solve_device(acc, shape):
    """hgs_field_solve: (dir f64 [nz, ny, nx, 3], conf f64 [nz, ny, nx]) on the device of acc."""
    import torch
    import hgs_runtime as rt
    nx, ny, nz = (int(n) for n in shape)
    rt.trace_check(acc, (nx, ny, nz))
    d = torch.empty((nz, ny, nx, 3), dtype=torch.float64, device=acc.device)
    conf = torch.empty((nz, ny, nx), dtype=torch.float64, device=acc.device)
    with torch.cuda.device(acc.device):
        rt.check(rt.lib().hgs_field_solve(rt.current_stream(), nx, ny, nz, rt.ptr(acc), rt.ptr(d), rt.ptr(conf)))
    return d, conf


def build_field(points, dirs, origin, h, shape, r, device=None, stats=None):
    """The Field of a directed cloud (host arrays).  `stats`, a dict, receives "skipped", "nonempty" and, where the key "acc" is
    present, the int64 sums."""
    origin, h, shape = check_grid(origin, h, shape)
    if is_cuda(device):
        import torch
        pts = torch.from_numpy(_rows3(points, "points")).to(device)
        dr = torch.from_numpy(_rows3(dirs, "dirs")).to(device)
        acc, skipped = splat_device(pts, dr, origin, h, shape, r)
        d, conf = solve_device(acc, shape)
        skipped = int(skipped.cpu()[0])
        acc_h = acc.cpu().numpy() if stats is not None and "acc" in stats else None
        nonempty = int((acc[..., 0] != 0).sum())
        d, conf = d.cpu().numpy(), conf.cpu().numpy()
    else:
        acc_h, skipped = splat_numpy(points, dirs, origin, h, shape, r)
        d, conf = solve_numpy(acc_h)
        nonempty = int((acc_h[..., 0] != 0).sum())
    if stats is not None:
        want_acc = "acc" in stats
        stats.update(skipped=skipped, nonempty=nonempty)
        if want_acc:
            stats["acc"] = acc_h
    return Field(origin, h, shape, d, conf)


def exclude_head(field, sdf, margin=0.0):
    """conf = 0 at the nodes whose interpolated head distance (utils.head_sdf.sample) is < margin; returns how many nodes that were
    not empty it cleared.  Host arithmetic, the same on both paths."""
    from utils.head_sdf import sample
    d = sample(field.nodes().astype(np.float32), sdf, 0.0)[2].reshape(field.conf.shape)
    inside = d < np.float32(margin)
    cleared = int((inside & (field.conf != 0)).sum())
    field.conf[inside] = 0.0
    return cleared


def save_field(path, field):
    np.savez(path, origin=field.origin, spacing=np.float64(field.spacing), shape=np.asarray(field.shape, np.int64), dir=field.dir,
             conf=field.conf)


def load_field(path):
    with np.load(path, allow_pickle=False) as z:
        if set(z.files) != set(FIELD_KEYS):
            raise ValueError(f"{path}: keys {sorted(z.files)}, a direction volume holds {sorted(FIELD_KEYS)}")
        return Field(z["origin"], float(z["spacing"]), tuple(int(v) for v in z["shape"]), z["dir"], z["conf"])


# ---- the trace -------------------------------------------------------------------------------------------------------------
def _check_knobs(step, max_steps, cos_max, min_conf, max_gap):
    step, cos_max, min_conf = float(step), float(cos_max), float(min_conf)
    if int(max_steps) != max_steps or not 1 <= max_steps <= MAX_STEPS or int(max_gap) != max_gap or max_gap < 0:
        raise ValueError(f"max_steps = {max_steps} (an integer, 1 to {MAX_STEPS}), max_gap = {max_gap} (an integer >= 0)")
    if not (math.isfinite(step) and step > 0.0 and -1.0 <= cos_max <= 1.0 and math.isfinite(min_conf)):
        raise ValueError(f"step = {step} (finite and > 0), cos_max = {cos_max} (-1 to 1), min_conf = {min_conf} (finite)")
    return step, int(max_steps), cos_max, min_conf, int(max_gap)


def trace_numpy(roots, p0, field, step, max_steps, cos_max, min_conf, max_gap):
    """(joints f64 [S, max_steps + 1, 3], count i32 [S], reason i32 [S]) of the contract's loop, vectorised over the strands that are
    still alive; rows of joints from count on are zero or coasted joints."""
    roots, p0 = _rows3(roots, "roots"), _rows3(p0, "p0")
    step, max_steps, cos_max, min_conf, max_gap = _check_knobs(step, max_steps, cos_max, min_conf, max_gap)
    S = roots.shape[0]
    if p0.shape[0] != S or S > MAX_ROOTS:
        raise ValueError(f"{S} roots with {p0.shape[0]} initial directions (equal counts, at most 2^24)")
    nx, ny, nz = field.shape
    o, k = field.origin, 1.0 / field.spacing
    top = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    dirf, conff = field.dir.reshape(-1, 3), field.conf.reshape(-1)
    joints = np.zeros((S, max_steps + 1, 3), np.float64)
    joints[:, 0] = roots
    reason = np.full(S, STEPS, np.int32)
    last, gap, entered = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, bool)
    x, p = roots.copy(), p0.copy()
    live = np.arange(S)
    with np.errstate(all="ignore"):
        for it in range(max_steps):
            if live.size == 0:
                break
            t = (x[live] - o[None, :]) * k
            ok = ((t >= 0.0) & (t < top[None, :])).all(axis=1)               # (a NaN fails every comparison, +inf the second)
            reason[live[~ok]] = BOUNDS
            live, t = live[ok], t[ok]
            if live.size == 0:
                break
            pa = p[live]
            fl = np.floor(t)
            i = fl.astype(np.int64)
            f = t - fl
            g = 1.0 - f
            base = (i[:, 2] * ny + i[:, 1]) * nx + i[:, 0]
            w = np.zeros(live.size, np.float64)
            v = [np.zeros(live.size, np.float64) for _ in range(3)]
            for cz in (0, 1):
                for cy in (0, 1):
                    for cx in (0, 1):
                        at = base + (cz * ny + cy) * nx + cx
                        tw = ((f[:, 0] if cx else g[:, 0]) * (f[:, 1] if cy else g[:, 1])) * (f[:, 2] if cz else g[:, 2])
                        a = tw * conff[at]
                        w = w + a
                        e = dirf[at]
                        a = np.where(_dot(e.T, pa.T) < 0.0, -a, a)
                        v = [v[j] + a * e[:, j] for j in range(3)]
            nn = _dot(v, v)
            on = (w >= min_conf) & np.isfinite(nn) & (nn > 0.0)
            ln = np.sqrt(nn)
            d = np.stack([v[j] / ln for j in range(3)], axis=1)
            turn = on & entered[live] & (_dot(d.T, pa.T) < cos_max)
            gap_new = np.where(on, 0, gap[live] + 1)
            lost = ~on & (gap_new > max_gap)
            reason[live[turn]] = TURN
            reason[live[lost]] = GAP
            go = ~(turn | lost)
            entered[live[on & go]] = True
            gap[live] = gap_new
            d = np.where(on[:, None], d, pa)
            live, d, gap_new = live[go], d[go], gap_new[go]
            x[live] = x[live] + step * d
            p[live] = d
            joints[live, it + 1] = x[live]
            last[live] = np.where(gap_new == 0, it + 1, last[live])
    return joints, (last + 1).astype(np.int32), reason


def trace_device(roots, p0, dir, conf, origin, h, shape, step, max_steps, cos_max, min_conf, max_gap):
    """hgs_strand_trace on float64 device tensors: (joints [S, max_steps + 1, 3], count i32 [S], reason i32 [S]) on their device."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(roots, "roots", torch.float64)
    rt.require_device_buffer(p0, "p0", torch.float64)
    if roots.dim() != 2 or roots.shape[1] != 3 or tuple(p0.shape) != tuple(roots.shape):
        raise rt.HgsError(f"roots {tuple(roots.shape)} and p0 {tuple(p0.shape)}: [S, 3] both expected")
    try:
        origin, h, (nx, ny, nz) = check_grid(origin, h, shape)
        step, max_steps, cos_max, min_conf, max_gap = _check_knobs(step, max_steps, cos_max, min_conf, max_gap)
    except ValueError as e:
        raise rt.HgsError(str(e)) from None
    rt.trace_check(shape=(nx, ny, nz), dir=dir, conf=conf)
    S = roots.shape[0]
    joints = torch.empty((S, max_steps + 1, 3), dtype=torch.float64, device=roots.device)
    count = torch.empty(S, dtype=torch.int32, device=roots.device)
    reason = torch.empty(S, dtype=torch.int32, device=roots.device)
    with torch.cuda.device(roots.device):
        rt.check(rt.lib().hgs_strand_trace(rt.current_stream(), S, rt.ptr(roots), rt.ptr(p0), rt.ptr(dir), rt.ptr(conf), float(origin[0]),
                                           float(origin[1]), float(origin[2]), h, nx, ny, nz, step, max_steps, cos_max, min_conf, max_gap,
                                           rt.ptr(joints), rt.ptr(count), rt.ptr(reason)))
    return joints, count, reason


def batch_roots(max_steps, budget=BUDGET):
    """Roots per batch: their joints, 24 (max_steps + 1) bytes a root, fit `budget` bytes (at least one root)."""
    return max(1, int(budget) // (24 * (int(max_steps) + 1)))


def trace(roots, p0, field, step, max_steps, cos_max, min_conf, max_gap, device=None, budget=BUDGET):
    """The trace of host arrays, in batches of batch_roots(max_steps, budget) roots (a root's strand does not depend on the others):
    (joints, count, reason) as host arrays."""
    roots, p0 = _rows3(roots, "roots"), _rows3(p0, "p0")
    _check_knobs(step, max_steps, cos_max, min_conf, max_gap)
    S, B = roots.shape[0], batch_roots(max_steps, budget)
    if p0.shape[0] != S or S > MAX_ROOTS:
        raise ValueError(f"{S} roots with {p0.shape[0]} initial directions (equal counts, at most 2^24)")
    cuda = is_cuda(device)
    if cuda:
        import torch
        d_dev, c_dev = torch.from_numpy(field.dir).to(device), torch.from_numpy(field.conf).to(device)
    out = []
    for s0 in range(0, S, B):
        if cuda:
            got = trace_device(torch.from_numpy(roots[s0:s0 + B]).to(device), torch.from_numpy(p0[s0:s0 + B]).to(device), d_dev, c_dev,
                               field.origin, field.spacing, field.shape, step, max_steps, cos_max, min_conf, max_gap)
            out.append(tuple(t.cpu().numpy() for t in got))
        else:
            out.append(trace_numpy(roots[s0:s0 + B], p0[s0:s0 + B], field, step, max_steps, cos_max, min_conf, max_gap))
    if not out:
        return np.zeros((0, int(max_steps) + 1, 3), np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32)
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


# ---- host arithmetic shared by both paths (the driver's) ---------------------------------------------------------------------
def initial_directions(roots, head_verts):
    """p0 = unit(root - mean(head_verts)); a root at the mean gets +z."""
    roots = _rows3(roots, "roots")
    head = _rows3(head_verts, "head_verts")
    c = head[np.isfinite(head).all(axis=1)].mean(axis=0) if head.shape[0] else np.zeros(3)
    v = roots - c[None, :]
    with np.errstate(all="ignore"):
        n = np.sqrt(_dot(v.T, v.T))
        p = v / n[:, None]
    p[~(np.isfinite(p).all(axis=1) & (n > 0.0))] = (0.0, 0.0, 1.0)
    return p


def grid_box(points, roots, grid, r_voxels):
    """(origin, h, shape) of the driver's grid: the bounding box of the finite points and roots with `grid` nodes along its longest
    side, then padded by r + h on every side (r = r_voxels*h)."""
    grid = int(grid)
    pts = np.concatenate([_rows3(points, "points"), _rows3(roots, "roots")])
    pts = pts[np.isfinite(pts).all(axis=1)]
    if pts.shape[0] == 0:
        raise ValueError("no finite point or root to put a grid around")
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    pad_nodes = int(math.ceil(float(r_voxels))) + 1
    inner = grid - 2 * pad_nodes
    if inner < 2 or grid > 1024:
        raise ValueError(f"grid = {grid} with a radius of {r_voxels} voxels: {2 * pad_nodes + 2} to 1024")
    h = float((hi - lo).max() / (inner - 1))
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError(f"the box {lo.tolist()} .. {hi.tolist()} gives a spacing of {h}: a cloud with some extent expected")
    origin = lo - pad_nodes * h
    n = np.ceil((hi - lo) / h).astype(np.int64) + 1 + 2 * pad_nodes
    return check_grid(origin, h, tuple(int(v) for v in np.minimum(n, 1024)))


def lengths(joints, count):
    """Arc length f64 [S] of the first count joints of every strand (segments summed in order)."""
    seg = np.sqrt(((joints[:, 1:] - joints[:, :-1]) ** 2).sum(axis=2))
    seg = np.where(np.arange(seg.shape[1])[None, :] < (np.asarray(count)[:, None] - 1), seg, 0.0)
    return seg.sum(axis=1)


def resample(joints, count, points):
    """f64 [S, points, 3]: every strand (count >= 2) resampled to `points` joints at uniform arc length, the ends kept."""
    points = int(points)
    if points < 2:
        raise ValueError(f"points = {points}: at least 2")
    S = joints.shape[0]
    out = np.zeros((S, points, 3), np.float64)
    u = np.arange(points, dtype=np.float64) / (points - 1)
    for s in range(S):
        c = int(count[s])
        if c < 2:
            raise ValueError(f"strand {s} has {c} joint(s): at least 2 to resample")
        J = joints[s, :c]
        cum = np.concatenate([[0.0], np.cumsum(np.sqrt(((J[1:] - J[:-1]) ** 2).sum(axis=1)))])
        for a in range(3):
            out[s, :, a] = np.interp(u * cum[-1], cum, J[:, a])
        out[s, 0], out[s, -1] = J[0], J[-1]
    return out
