"""Guide strands picked from an exported groom (export_strands.py --select_guides): the export chain goes from few strands to many --
it resamples, roots, smooths, interpolates and pushes out of the head -- and every consumer that simulates a groom (engine grooms,
hair curves, mass-spring and rod solvers) wants the opposite step: a small set of guide strands, and a binding that tells every
rendered strand which guide it follows.  --interpolate --roots N samples roots evenly and knows nothing of a strand's shape, and a
decimation by index puts two guides on one lock and none on the next.  This is Lloyd's k-means over the strands' shapes, with each
cluster's most central MEMBER -- a real strand, not the shrunken mean -- as its guide.

The contract (this module's numpy path, csrc/hgs_guides.hip and the loop restatement in tests/guides_reference.py state the same
thing).  All arithmetic is float64 on the float32 inputs, with one rounding per operation, in exactly the order written (the kernel
file is built with -ffp-contract=off).

Inputs.  points float32 [N*M, 3].  offsets int64 [N + 1] (strand_collide.check_offsets): every strand has the same number M >= 2 of
points (strand_points raises ValueError for ragged strands, the device wrapper HgsError; the driver says that --points M > 0 is
needed).  k 1..65536.  samples 2..64, default 16.  iters 1..256, default 10.

Features.  S = min(samples, M).  Sample s is point j_s = (s*(M-1)) // (S-1), in integers.  Strand i's feature x_i is its S sampled
points as doubles.

Status.  A strand with any coordinate that is not finite among ALL its M points is NONFINITE (1): label -1, dist2 +inf, and it takes
part in nothing.  The others are ELIGIBLE (0); E lists them in ascending index, n_E of them.  K = min(k, n_E); n_E == 0 gives a result
without clusters.

Seeds.  c_k = x_{E[((2k+1)*n_E) // (2K)]} for k = 0 .. K-1, in integers.

Assignment.  d2(i, k) is accumulated from 0.0 over s = 0 .. S-1 in order: acc = acc + ((dx*dx + dy*dy) + dz*dz) with dx = x_i[s].x -
c_k[s].x and so on.  label_i is the k smallest by (d2, k): ties go to the smaller k.  dist2_i is that d2.  With finite float32 inputs
nothing overflows: at most 192 terms, each below 2^259.

Update.  For every cluster with members, each coordinate of c_k becomes the sum of the members' coordinates, added from 0.0 in
ascending strand index, divided by the member count as a double.  An empty cluster keeps its centroid.

Loop.  At most iters assignments, an update between two of them.  After assignment t >= 2, if every label equals the previous
assignment's, stop with converged = True.  The labels and dist2 of the last assignment are the result.

Pick.  guide_k is the member of cluster k smallest by (dist2_i, i); an empty cluster has guide -1.

Outputs (Guides).  labels int32 [N], dist2 float64 [N], guide int64 [K], count int32 [K], status int32 [N], iterations (assignments
run), converged; also centroids float64 [K, S, 3] (those the last assignment ran against) and first_dist2 float64 [N] (the first
assignment's dist2, for the report).

Known limits.  The metric is plain L2 on the sampled joints: there is no curvature term, and two locks of one shape at one place but
different frizz are one cluster.  The defaults are knobs, not measured optima.  Seeds are deterministic by index, not k-means++, and
duplicate seeds leave a cluster empty (it is skipped, so fewer than k guides can come back).  The process is Lloyd's: it reaches a
local optimum only, and `iters` may end it before that.  There are no binding weights and no secondary guides: a strand follows one
guide.

device=None: numpy, in chunks of strands against all centroids under a fixed element budget (BUDGET, like strand_export._BUDGET).
device="cuda": hgs_guides_assign / hgs_guides_update / hgs_guides_pick on torch tensors, the member list by a stable torch.sort of the
labels; the host reads one word per iteration, the count of changed labels.  The caller chooses; neither falls back to the other."""
from typing import NamedTuple

import numpy as np

from scene.strand_collide import _check_points, check_offsets
from scene.strand_export import StrandExport

ELIGIBLE, NONFINITE = range(2)
MAX_K, MAX_SAMPLES, MAX_ITERS = 65536, 64, 256
BUDGET = 1 << 21           # elements of one vectorised block of the numpy path (strands x centroids)


class Guides(NamedTuple):
    labels: np.ndarray       # int32 [N]: the strand's cluster, -1 for a NONFINITE strand
    dist2: np.ndarray        # float64 [N]: d2 to that cluster's centroid, +inf for a NONFINITE strand
    guide: np.ndarray        # int64 [K]: the cluster's guide strand, -1 for an empty cluster
    count: np.ndarray        # int32 [K]: the cluster's members
    status: np.ndarray       # int32 [N]: ELIGIBLE / NONFINITE
    iterations: int          # assignments run
    converged: bool
    centroids: np.ndarray    # float64 [K, S, 3]: what the last assignment ran against
    first_dist2: np.ndarray  # float64 [N]: dist2 of the first assignment


def check_parameters(k, samples=16, iters=10):
    """(k, samples, iters) of the contract as ints, or ValueError."""
    for name, v, lo, hi in (("k", k, 1, MAX_K), ("samples", samples, 2, MAX_SAMPLES), ("iters", iters, 1, MAX_ITERS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{name} = {v}: {lo} to {hi}")
    return int(k), int(samples), int(iters)


def strand_points(offsets):
    """M, the number of points every strand has (0 where there is no strand), or ValueError for ragged or one-point strands."""
    off = np.asarray(offsets, np.int64)
    n = off[1:] - off[:-1]
    if n.shape[0] == 0:
        return 0
    M = int(n[0])
    if np.any(n != M) or M < 2:
        raise ValueError(f"strands of {int(n.min())} to {int(n.max())} points: every strand must have the same number M >= 2 of points "
                         "(resample them first)")
    return M


def sample_joints(M, S):
    """j_s = (s*(M-1)) // (S-1), int64 [S]."""
    return (np.arange(S, dtype=np.int64) * (M - 1)) // (S - 1)


def seed_strands(n_E, K):
    """The positions in E of the K seeds: ((2k+1)*n_E) // (2K), int64 [K]."""
    return ((2 * np.arange(K, dtype=np.int64) + 1) * n_E) // (2 * K)


def _empty(N, status, S):
    return Guides(np.full(N, -1, np.int32), np.full(N, np.inf), np.zeros(0, np.int64), np.zeros(0, np.int32), status, 0, False,
                  np.zeros((0, S, 3)), np.full(N, np.inf))


# ---- numpy path ------------------------------------------------------------------------------------------------------------------
def assign_numpy(x, cent, budget=BUDGET):
    """(label int32 [n], dist2 float64 [n]) of the features x [n, S, 3] against the centroids cent [K, S, 3], both float64: the
    contract's assignment, `budget` // K strands at a time."""
    n, S, K = x.shape[0], x.shape[1], cent.shape[0]
    label, dist2 = np.zeros(n, np.int32), np.zeros(n, np.float64)
    step = max(1, int(budget) // K)
    for a in range(0, n, step):
        xa = x[a:a + step]
        acc = np.zeros((xa.shape[0], K), np.float64)
        for s in range(S):
            dx = xa[:, None, s, 0] - cent[None, :, s, 0]
            dy = xa[:, None, s, 1] - cent[None, :, s, 1]
            dz = xa[:, None, s, 2] - cent[None, :, s, 2]
            acc = acc + ((dx * dx + dy * dy) + dz * dz)
        best = np.argmin(acc, axis=1)                                               # (the first of equal minima: the smaller k)
        label[a:a + step] = best
        dist2[a:a + step] = acc[np.arange(xa.shape[0]), best]
    return label, dist2


def update_numpy(x, label, cent):
    """The contract's update of cent [K, S, 3] (a new array) from the features x [n, S, 3] in ascending strand index and their labels,
    and count int32 [K]."""
    K, S = cent.shape[0], cent.shape[1]
    sums = np.zeros((K, 3 * S), np.float64)
    np.add.at(sums, label, x.reshape(x.shape[0], 3 * S))                            # unbuffered: row after row, in order, from 0.0
    count = np.bincount(label, minlength=K).astype(np.int32)
    out = cent.copy()
    has = count > 0
    out[has] = (sums[has] / count[has].astype(np.float64)[:, None]).reshape(-1, S, 3)
    return out, count


def pick_numpy(E, label, dist2, K):
    """(guide int64 [K], count int32 [K]): per cluster the member smallest by (dist2, i) among the strands E (ascending) with the
    labels and dist2 given for them; -1 for an empty cluster."""
    count = np.bincount(label, minlength=K).astype(np.int32)
    order = np.lexsort((E, dist2, label))                                           # by label, then dist2, then strand index
    first = np.cumsum(count, dtype=np.int64) - count
    guide = np.full(K, -1, np.int64)
    has = count > 0
    guide[has] = E[order[first[has]]]
    return guide, count


def guides_numpy(points, offsets, k, samples=16, iters=10, budget=BUDGET):
    """Guides of the contract, by numpy."""
    points = _check_points(points)
    off = check_offsets(offsets, points.shape[0])
    k, samples, iters = check_parameters(k, samples, iters)
    N, M = off.shape[0] - 1, strand_points(off)
    S = min(samples, M) if N else samples
    if N == 0:
        return _empty(0, np.zeros(0, np.int32), S)
    p = points.reshape(N, M, 3)
    status = np.where(np.isfinite(p).all(axis=(1, 2)), ELIGIBLE, NONFINITE).astype(np.int32)
    E = np.nonzero(status == ELIGIBLE)[0]
    n_E = int(E.shape[0])
    K = min(k, n_E)
    if K == 0:
        return _empty(N, status, S)
    x = p[E][:, sample_joints(M, S)].astype(np.float64)                             # [n_E, S, 3]
    cent = x[seed_strands(n_E, K)].copy()
    label = prev = first = None
    converged, t = False, 0
    while t < iters:
        if t > 0:
            cent, _ = update_numpy(x, label, cent)
        prev = label
        label, d2 = assign_numpy(x, cent, budget)
        t += 1
        if t == 1:
            first = d2
        elif np.array_equal(label, prev):
            converged = True
            break
    guide, count = pick_numpy(E, label, d2, K)
    labels, dist2, first_dist2 = np.full(N, -1, np.int32), np.full(N, np.inf), np.full(N, np.inf)
    labels[E], dist2[E], first_dist2[E] = label, d2, first
    return Guides(labels, dist2, guide, count, status, t, converged, cent, first_dist2)


# ---- device path -----------------------------------------------------------------------------------------------------------------
def _strands_of(rt, points, offsets):
    """(points, N, M) of device tensors points float32 [N*M, 3] and offsets int64 [N + 1], or HgsError (one synchronisation)."""
    import torch
    points = rt.require_gpu_tensor(points, "points", torch.float32)
    offsets = rt.require_gpu_tensor(offsets, "offsets", torch.int64)
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise rt.HgsError(f"guides_device: points {tuple(points.shape)} and offsets {tuple(offsets.shape)}; [N*M, 3] and [N + 1] expected")
    N = int(offsets.shape[0]) - 1
    if N == 0:
        return points, 0, 0
    n = offsets[1:] - offsets[:-1]
    M, lo, hi, a, b = (int(v) for v in torch.stack([n[0], n.min(), n.max(), offsets[0], offsets[-1]]).tolist())
    if lo != hi or M < 2 or a != 0 or b != points.shape[0]:
        raise rt.HgsError(f"guides_device: strands of {lo} to {hi} points over {b - a} of {points.shape[0]} points: every strand must have "
                          "the same number M >= 2 of points, and the offsets must tile the points")
    return points, N, M


def member_list(labels, K):
    """(order int64 [n], start int64 [K + 1]) of device labels int32 [N]: the strands that have a label, by label and within one in
    ascending index (a stable sort), and the clusters' ranges in that list."""
    import torch
    vals, order = torch.sort(labels, stable=True)
    skip = torch.searchsorted(vals, torch.zeros(1, dtype=vals.dtype, device=vals.device))      # the strands labelled -1 come first
    vals, order = vals[int(skip):].contiguous(), order[int(skip):].contiguous()
    start = torch.searchsorted(vals, torch.arange(K + 1, dtype=vals.dtype, device=vals.device)).to(torch.int64).contiguous()
    return order, start


def assign_device(points, N, M, S, status, cent, prev=None, changed=None):
    """hgs_guides_assign on device tensors: (label int32 [N], dist2 float64 [N]); `changed` (int32 [1], added to) with `prev`."""
    import torch
    import hgs_runtime as rt
    label = torch.empty(N, dtype=torch.int32, device=points.device)
    dist2 = torch.empty(N, dtype=torch.float64, device=points.device)
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_guides_assign(rt.current_stream(), N, M, S, int(points.shape[0]), rt.ptr(points), rt.ptr(status), int(cent.shape[0]),
                                            rt.ptr(cent), None if prev is None else rt.ptr(prev), rt.ptr(label), rt.ptr(dist2),
                                            None if changed is None else changed.data_ptr()))
    return label, dist2


def update_device(points, N, M, S, order, start, cent):
    """hgs_guides_update on device tensors: cent float64 [K, S, 3] is updated in place; returns count int32 [K]."""
    import torch
    import hgs_runtime as rt
    K = int(cent.shape[0])
    count = torch.empty(K, dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_guides_update(rt.current_stream(), N, M, S, int(points.shape[0]), rt.ptr(points), K, rt.ptr(order),
                                            int(order.shape[0]), rt.ptr(start), rt.ptr(cent), rt.ptr(count)))
    return count


def pick_device(N, K, order, start, dist2):
    """hgs_guides_pick on device tensors: guide int64 [K]."""
    import torch
    import hgs_runtime as rt
    guide = torch.empty(K, dtype=torch.int64, device=dist2.device)
    with torch.cuda.device(dist2.device):
        rt.check(rt.lib().hgs_guides_pick(rt.current_stream(), N, K, rt.ptr(order), int(order.shape[0]), rt.ptr(start), rt.ptr(dist2),
                                          rt.ptr(guide)))
    return guide


def guides_device(points, offsets, k, samples=16, iters=10):
    """Guides of the contract by the HIP kernels, on device tensors points float32 [N*M, 3] and offsets int64 [N + 1]; the result's
    arrays are copied to the host."""
    import torch
    import hgs_runtime as rt
    points, N, M = _strands_of(rt, points, offsets)
    try:
        k, samples, iters = check_parameters(k, samples, iters)
    except ValueError as e:
        raise rt.HgsError(f"guides_device: {e}") from None
    S = min(samples, M) if N else samples
    dev = points.device
    if N == 0:
        return _empty(0, np.zeros(0, np.int32), S)
    status = (~torch.isfinite(points.view(N, M * 3)).all(dim=1)).to(torch.int32)
    E = torch.nonzero(status == ELIGIBLE).flatten()
    n_E = int(E.shape[0])
    K = min(k, n_E)
    if K == 0:
        return _empty(N, status.cpu().numpy(), S)
    joints = torch.as_tensor(sample_joints(M, S), device=dev)
    seeds = E[torch.as_tensor(seed_strands(n_E, K), device=dev)]
    cent = points.view(N, M, 3)[seeds][:, joints].to(torch.float64).contiguous()    # [K, S, 3]
    changed = torch.zeros(iters, dtype=torch.int32, device=dev)
    label = first = None
    converged, t = False, 0
    while t < iters:
        if t > 0:
            update_device(points, N, M, S, *member_list(label, K), cent)
        prev = label
        label, d2 = assign_device(points, N, M, S, status, cent, prev, None if prev is None else changed[t:t + 1])
        t += 1
        if t == 1:
            first = d2
        elif int(changed[t - 1]) == 0:                                              # the loop's only synchronisation
            converged = True
            break
    order, start = member_list(label, K)
    guide = pick_device(N, K, order, start, d2)
    count = (start[1:] - start[:-1]).to(torch.int32)
    return Guides(label.cpu().numpy(), d2.cpu().numpy(), guide.cpu().numpy(), count.cpu().numpy(), status.cpu().numpy(), t, converged,
                  cent.cpu().numpy(), first.cpu().numpy())


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def report_of(res, k, S):
    """The report of select_guides from the host arrays of either path: one set of numpy statements for both."""
    ok = res.status == ELIGIBLE
    size = res.count[res.count > 0].astype(np.float64)
    dist = np.sqrt(res.dist2[ok] / float(S))
    return dict(strands=int(res.status.shape[0]), eligible=int(ok.sum()), nonfinite=int((~ok).sum()), clusters_asked=int(k),
                clusters_made=int(res.count.shape[0]), clusters_empty=int((res.count == 0).sum()), iterations=int(res.iterations),
                converged=bool(res.converged), size_min=int(size.min()) if size.shape[0] else 0,
                size_mean=float(size.mean()) if size.shape[0] else 0.0, size_max=int(size.max()) if size.shape[0] else 0,
                distance_mean=float(dist.mean()) if dist.shape[0] else 0.0, distance_max=float(dist.max()) if dist.shape[0] else 0.0,
                total_first=float(res.first_dist2[ok].sum()), total_last=float(res.dist2[ok].sum()))


def binding_of(res, S):
    """The binding of select_guides from a Guides: guide_strand int64 [G] (an index into the input strands, ascending cluster order,
    empty clusters skipped), strand_guide int32 [N] (an index into the guides, or -1), strand_distance float64 [N] = sqrt(dist2 / S),
    the RMS joint distance to the centroid (+inf for a NONFINITE strand), cluster_size int32 [G]."""
    used = res.guide >= 0
    remap = np.full(res.guide.shape[0] + 1, -1, np.int32)                           # (the last entry serves label -1)
    remap[:-1][used] = np.arange(int(used.sum()), dtype=np.int32)
    return dict(guide_strand=res.guide[used].astype(np.int64), strand_guide=remap[res.labels].astype(np.int32),
                strand_distance=np.sqrt(res.dist2 / float(S)), cluster_size=res.count[used].astype(np.int32))


def select_guides(strands, k, samples=16, iters=10, device=None, budget=BUDGET):
    """Guide strands picked from `strands` (a StrandExport of strands with the same number of points), see the module docstring:
    (guides, binding, report).  guides: a StrandExport of the guide strands in ascending cluster order, empty clusters skipped, every
    bit of their points, attributes, ids and lengths kept.  binding: binding_of.  report: "strands", "eligible", "nonfinite",
    "clusters_asked", "clusters_made", "clusters_empty", "iterations", "converged", "size_min", "size_mean", "size_max" (over the clusters
    that have members), "distance_mean", "distance_max" (strand_distance over the eligible strands), "total_first" and "total_last" (the
    sum of dist2 over the eligible strands after the first and after the last assignment).  device=None: numpy; "cuda": the HIP kernels."""
    points = _check_points(strands.points)
    off = check_offsets(strands.offsets, points.shape[0])
    k, samples, iters = check_parameters(k, samples, iters)
    M = strand_points(off)
    S = min(samples, M) if M else samples
    if device is None:
        res = guides_numpy(points, off, k, samples, iters, budget)
    else:
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernels)")
        import torch
        res = guides_device(torch.as_tensor(points, device=device), torch.as_tensor(off, device=device), k, samples, iters)
    binding = binding_of(res, S)
    g = binding["guide_strand"]
    rows = (off[g][:, None] + np.arange(M, dtype=np.int64)[None, :]).reshape(-1)
    guides = StrandExport(points[rows], np.asarray(strands.attrs)[rows], np.arange(g.shape[0] + 1, dtype=np.int64) * M,
                          np.asarray(strands.strand_ids)[g], np.asarray(strands.length)[g])
    return guides, binding, report_of(res, k, S)
