"""The direction volume of utils/trace.py filled between the scalp and the visible hair: the known orientations are held fixed where
the volume has data, the interior is their harmonic interpolation, relaxed on the sign-free tensors d d^T (the classical inward
diffusion of a volumetric multi-view orientation field).  trace_strands.py --fill N is the scene driver.  The reference has no such step.

The contract (this module's numpy path, csrc/hgs_fill.hip and the loop restatement in tests/fill_reference.py state the same thing).
All arithmetic is float64 with one rounding per operation, in exactly the order written (the kernel file is built with
-ffp-contract=off).  Arrays are laid out as in utils/trace.py; the tensor planes come first, T f64 [6, nz, ny, nx] in the order xx, xy,
xz, yy, yz, zz, so that a node's six values are six coalesced plane reads.

Kinds.  kind uint8 [nz, ny, nx]: OUT = 0, FREE = 1, FIXED = 2.  classify(field, fixed_conf, allowed): a node is FIXED iff conf >=
fixed_conf and its dir is finite; FREE iff it is not FIXED and `allowed` (bool [nz, ny, nx]; None: everywhere) is true there; every
other node is OUT.

Seed.  seed(field, kind): the six products d_a*d_b of dir at the FIXED nodes (unit-trace tensors: the node's conf is dropped on
purpose), +0.0 everywhere else.  Negating a dir changes no bit.

Sweep (Jacobi).  A FREE node computes from the previous iterate T_old, per entry ab:
    s = 0.0, c = 0;  the six face neighbours in the order -x, +x, -y, +y, -z, +z:
       on the grid and not OUT:   s = s + T_old_ab[neighbour],  c = c + 1
       off the grid or OUT:       s = s + 0.0                    (performed: a -0.0 sum behaves alike on every path)
    T_new_ab = s / (double)c  if c > 0,  else T_old_ab
FIXED and OUT nodes never change.  OUT neighbours do not count: the domain's border is a no-flux border.  fill(T, kind, sweeps)
returns the iterate after `sweeps` sweeps and the one before it; 0 <= sweeps <= 65536 (MAX_SWEEPS), and sweeps = 0 returns T twice.

Back to a field.  quantise(T) gives acc int64 [nz, ny, nx, 7] = (W, xx, xy, xz, yy, yz, zz): Wq = rint(((Txx + Tyy) + Tzz) * 2^32),
Tq_ab = rint(T_ab * 2^32), round-half-even.  The values are convex combinations of unit-trace tensors, so they fit; a T that is not
finite is refused.  The solve of utils/trace.py (solve_numpy / solve_device, unchanged) turns acc into dir and conf as it does for the
splat, and merge(field, kind, dir_f, conf_f) writes them into the FREE nodes only: every FIXED and OUT node keeps its bits.  At a
filled node conf = l2 - l1 lies in [0, 1]: anisotropy times how far the relaxation has come, so the tracer's --min_conf applies to it
unchanged.

Equality.  The kernel, the numpy path and the loop give equal bits in T for any kind and any sweeps: addition and division are
correctly rounded on both sides and the order is fixed.  The solve afterwards agrees under tests/trace_reference.compare_solves.

Known limits.  Plain Jacobi needs on the order of L^2 sweeps for a gap of L voxels; there is no multigrid.  The hull domain is only as
good as the masks.  The scalp condition is the radial direction unit(root - head centre), not a mesh normal.

device=None: numpy.  device="cuda": the kernel.  The caller chooses; neither falls back to the other."""
import numpy as np

from utils.trace import FIXED_ONE, Field, solve_device, solve_numpy
from utils.views import is_cuda

OUT, FREE, FIXED = 0, 1, 2
MAX_SWEEPS = 65536
_PRODUCTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
_STEPS = ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))       # (axis, step): -x, +x, -y, +y, -z, +z


def _check_kind(kind, shape):
    nx, ny, nz = shape
    kind = np.asarray(kind)
    if kind.dtype != np.uint8 or kind.shape != (nz, ny, nx):
        raise ValueError(f"kind {kind.shape} {kind.dtype}: uint8 [{nz}, {ny}, {nx}] expected")
    if kind.size and int(kind.max()) > FIXED:
        raise ValueError(f"kind holds the value {int(kind.max())}: OUT = 0, FREE = 1, FIXED = 2")
    return np.ascontiguousarray(kind)


def _check_sweeps(sweeps):
    if int(sweeps) != sweeps or not 0 <= sweeps <= MAX_SWEEPS:
        raise ValueError(f"sweeps = {sweeps} (an integer, 0 to {MAX_SWEEPS})")
    return int(sweeps)


def _check_planes(T):
    T = np.asarray(T)
    if T.dtype != np.float64 or T.ndim != 4 or T.shape[0] != 6:
        raise ValueError(f"T {T.shape} {T.dtype}: float64 [6, nz, ny, nx] expected")
    return np.ascontiguousarray(T)


def classify(field, fixed_conf, allowed=None):
    """kind uint8 [nz, ny, nx] of the contract."""
    nx, ny, nz = field.shape
    with np.errstate(all="ignore"):
        fixed = (field.conf >= float(fixed_conf)) & np.isfinite(field.dir).all(axis=-1)
    if allowed is None:
        free = ~fixed
    else:
        allowed = np.asarray(allowed)
        if allowed.dtype != np.bool_ or allowed.shape != (nz, ny, nx):
            raise ValueError(f"allowed {allowed.shape} {allowed.dtype}: bool [{nz}, {ny}, {nx}] expected")
        free = ~fixed & allowed
    kind = np.full((nz, ny, nx), OUT, np.uint8)
    kind[free] = FREE
    kind[fixed] = FIXED
    return kind


def counts(kind):
    """(fixed, free, out) node counts."""
    return int((kind == FIXED).sum()), int((kind == FREE).sum()), int((kind == OUT).sum())


def seed(field, kind):
    """T f64 [6, nz, ny, nx]: d_a*d_b at the FIXED nodes, +0.0 elsewhere."""
    kind = _check_kind(kind, field.shape)
    nx, ny, nz = field.shape
    T = np.zeros((6, nz, ny, nx), np.float64)
    fixed = kind == FIXED
    d = field.dir[fixed]
    for j, (a, b) in enumerate(_PRODUCTS):
        T[j][fixed] = d[:, a] * d[:, b]
    return T


def free_neighbours(kind):
    """(index int64 [F], neighbour int64 [6, F], valid bool [6, F], c int64 [F]) of the FREE nodes, ascending: the flat index of every
    face neighbour (the node's own where there is none to read) and whether it is on the grid and not OUT."""
    nz, ny, nx = kind.shape
    flat = kind.reshape(-1)
    index = np.nonzero(flat == FREE)[0].astype(np.int64)
    coord = [index % nx, (index // nx) % ny, index // (nx * ny)]
    size, stride = (nx, ny, nz), (1, nx, nx * ny)
    nbr, valid = np.empty((6, index.size), np.int64), np.empty((6, index.size), bool)
    for n, (axis, step) in enumerate(_STEPS):
        on = (coord[axis] + step >= 0) & (coord[axis] + step < size[axis])
        at = np.where(on, index + step * stride[axis], index)
        valid[n] = on & (flat[at] != OUT)
        nbr[n] = np.where(valid[n], at, index)
    return index, nbr, valid, valid.sum(axis=0)


def fill_numpy(T, kind, sweeps):
    """(the iterate after `sweeps` sweeps, the one before it), f64 [6, nz, ny, nx] both; over the compact list of FREE nodes, as the
    kernel."""
    T = _check_planes(T)
    nz, ny, nx = T.shape[1:]
    kind = _check_kind(kind, (nx, ny, nz))
    sweeps = _check_sweeps(sweeps)
    a, b = T.reshape(6, -1).copy(), T.reshape(6, -1).copy()
    index, nbr, valid, c = free_neighbours(kind)
    if index.size:
        some = c > 0
        cd = np.where(some, c, 1).astype(np.float64)
        for k in range(sweeps):
            src, dst = (a, b) if k % 2 == 0 else (b, a)
            for j in range(6):
                plane = src[j]
                s = np.zeros(index.size, np.float64)
                for n in range(6):
                    s = s + np.where(valid[n], plane[nbr[n]], 0.0)
                dst[j][index] = np.where(some, s / cd, plane[index])
    res, prev = (a, b) if sweeps % 2 == 0 else (b, a)
    return res.reshape(T.shape), prev.reshape(T.shape)


def fill_check_device(T, kind):
    """The grid (nx, ny, nz) of device tensors T f64 [6, nz, ny, nx] and kind uint8 [nz, ny, nx]; HgsError otherwise."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(T, "T", torch.float64)
    rt.require_device_buffer(kind, "kind", torch.uint8)
    if T.dim() != 4 or T.shape[0] != 6 or kind.dim() != 3 or tuple(T.shape[1:]) != tuple(kind.shape):
        raise rt.HgsError(f"T {tuple(T.shape)} and kind {tuple(kind.shape)}: [6, nz, ny, nx] and [nz, ny, nx] expected")
    nz, ny, nx = (int(n) for n in kind.shape)
    return nx, ny, nz


def fill_device(T, kind, sweeps):
    """hgs_field_fill on device tensors T f64 [6, nz, ny, nx] and kind uint8 [nz, ny, nx]: (result, previous) on their device, both
    new tensors.  `sweeps` launches are enqueued on the current stream with no host synchronisation between them."""
    import torch
    import hgs_runtime as rt
    nx, ny, nz = fill_check_device(T, kind)
    try:
        sweeps = _check_sweeps(sweeps)
    except ValueError as e:
        raise rt.HgsError(str(e)) from None
    a, b = T.clone(), T.clone()
    free_index = torch.nonzero(kind.reshape(-1) == FREE).reshape(-1).to(torch.int32)      # ascending
    F = rt.fill_check((nx, ny, nz), kind, a, b, free_index)
    with torch.cuda.device(T.device):
        rt.check(rt.lib().hgs_field_fill(rt.current_stream(), nx, ny, nz, rt.ptr(kind), rt.ptr(free_index), F, rt.ptr(a), rt.ptr(b), sweeps))
    return (a, b) if sweeps % 2 == 0 else (b, a)


def fill(T, kind, sweeps, device=None):
    """fill_numpy, or fill_device around host arrays: (result, previous) as host arrays."""
    if not is_cuda(device):
        return fill_numpy(T, kind, sweeps)
    import torch
    T = _check_planes(T)
    nz, ny, nx = T.shape[1:]
    kind = _check_kind(kind, (nx, ny, nz))
    _check_sweeps(sweeps)
    res, prev = fill_device(torch.from_numpy(T).to(device), torch.from_numpy(kind).to(device), sweeps)
    return res.cpu().numpy(), prev.cpu().numpy()


def quantise(T):
    """acc int64 [nz, ny, nx, 7] of the contract; ValueError for a T that is not finite."""
    T = _check_planes(T)
    if not np.isfinite(T).all():
        raise ValueError("T holds a value that is not finite: nothing to quantise")
    acc = np.empty(T.shape[1:] + (7,), np.int64)
    acc[..., 0] = np.rint(((T[0] + T[3]) + T[5]) * FIXED_ONE).astype(np.int64)
    for j in range(6):
        acc[..., j + 1] = np.rint(T[j] * FIXED_ONE).astype(np.int64)
    return acc


def quantise_device(T):
    """quantise on a device tensor (elementwise tensor arithmetic, float64: the same roundings): int64 [nz, ny, nx, 7]."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(T, "T", torch.float64)
    if T.dim() != 4 or T.shape[0] != 6:
        raise rt.HgsError(f"T {tuple(T.shape)}: [6, nz, ny, nx] expected")
    if not bool(torch.isfinite(T).all()):
        raise rt.HgsError("T holds a value that is not finite: nothing to quantise")
    acc = torch.empty(tuple(T.shape[1:]) + (7,), dtype=torch.int64, device=T.device)
    acc[..., 0] = torch.round(((T[0] + T[3]) + T[5]) * FIXED_ONE).to(torch.int64)
    for j in range(6):
        acc[..., j + 1] = torch.round(T[j] * FIXED_ONE).to(torch.int64)
    return acc


def merge(field, kind, dir_f, conf_f):
    """A new Field: dir_f and conf_f at the FREE nodes, the input's bits at every FIXED and OUT node."""
    kind = _check_kind(kind, field.shape)
    dir_f, conf_f = np.asarray(dir_f, np.float64), np.asarray(conf_f, np.float64)
    if dir_f.shape != field.dir.shape or conf_f.shape != field.conf.shape:
        raise ValueError(f"dir {dir_f.shape} and conf {conf_f.shape} for a field of dir {field.dir.shape} and conf {field.conf.shape}")
    free = kind == FREE
    d, conf = field.dir.copy(), field.conf.copy()
    d[free] = dir_f[free]
    conf[free] = conf_f[free]
    return Field(field.origin, field.spacing, field.shape, d, conf)


def fill_field(field, kind, sweeps, device=None, stats=None):
    """seed, fill, quantise, solve and merge in one: the filled Field (host arrays).  `stats`, a dict, receives "last_change", the
    largest absolute difference between the last iterate and the one before it."""
    T = seed(field, kind)
    if is_cuda(device):
        import torch
        res, prev = fill_device(torch.from_numpy(T).to(device), torch.from_numpy(_check_kind(kind, field.shape)).to(device), sweeps)
        change = float((res - prev).abs().max())
        d, conf = solve_device(quantise_device(res), field.shape)
        d, conf = d.cpu().numpy(), conf.cpu().numpy()
    else:
        res, prev = fill_numpy(T, kind, sweeps)
        change = float(np.abs(res - prev).max())
        d, conf = solve_numpy(quantise(res))
    if stats is not None:
        stats["last_change"] = change
    return merge(field, kind, d, conf)
