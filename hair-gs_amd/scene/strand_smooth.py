"""Exported strands smoothed without shrinking them (export_strands.py --smooth_strands): every joint of an exported strand is a
trained Gaussian endpoint, and endpoints jitter from segment to segment by a fraction of a millimetre.  Arc-length resampling only
re-spaces that jitter along the same piecewise-linear path, --attach_roots leaves a kink where the marched joints meet the strand's
own, --interpolate copies the guides' jitter onto every blended strand, and a consumer of a .hair / .data file computes its tangents
from neighbouring points, so it shades the jitter as frizz.  This is the low-pass over the polylines: Taubin's lambda|mu filter with
both end joints pinned, its weights taken from the original segment lengths so that one rule serves uniform (--points M) and ragged
(--points 0) strands.

The contract (this module's numpy path, csrc/hgs_strand_smooth.hip and the loop restatement in tests/smooth_reference.py state the
same thing).  It follows scene/strand_collide.py's conventions: all arithmetic is float64 on the float32 inputs, with one rounding
per operation, in exactly the order written; dot(u, v) = (u0*v0 + u1*v1) + u2*v2; results are rounded once to float32 (the kernel
file is built with -ffp-contract=off).

Inputs.  points float32 [P, 3].  offsets int64 [K + 1] (strand_collide.check_offsets).  iters 1..256, default 10.  lam float64,
default 0.5.  mu float64, default -0.53.  max_move None, or a finite float64 > 0.

Parameter check (check_parameters raises ValueError; the device wrapper raises HgsError).  0 < lam <= 1.  mu == 0 (plain Laplacian
smoothing, which shrinks), or -1 <= mu < -lam.  abs((1 - 2*lam) * (1 - 2*mu)) <= 1: the weighted operator's eigenvalues lie in
[0, 2], and this is the condition that no mode grows at the top of that range.

Per strand s with joints p_0 .. p_{n-1} as float64:
    status SHORT (1): n < 3.  LONG (2): n > MAX_JOINTS = 1024.  NONFINITE (3): any coordinate is not finite.  The strand is copied.
    Otherwise SMOOTHED (0):
    1.  e_i = p_{i+1} - p_i and l_i = sqrt(dot(e_i, e_i)), for i = 0 .. n-2.
    2.  For inner j = 1 .. n-2: s_j = l_{j-1} + l_j.  If s_j > 0: a_j = l_j / s_j and b_j = l_{j-1} / s_j.  Otherwise a_j = b_j = 0.5.
    3.  One sweep with factor f, Jacobi: every joint of sweep t+1 is computed from sweep t's joints only.  For every inner j and
        coordinate c:  m = a_j*x_{j-1}[c] + b_j*x_{j+1}[c];  x'_j[c] = x_j[c] + f*(m - x_j[c]).  x_0 and x_{n-1} stay.
    4.  Repeat iters times: a sweep with lam, then, unless mu == 0, a sweep with mu.
    5.  If max_move is given, for every inner j: u = x_j - p_j; du = sqrt(dot(u, u)); if du > max_move: x_j = p_j + (max_move/du)*u
        per coordinate, and clamped[s] += 1.
    6.  out_j = float32(x_j) for the inner joints.  The two end joints get their input bits.

Outputs.  out_points float32 [P, 3], status int32 [K], clamped int32 [K].

Consequences.  Roots and tips keep their bits, a copied strand keeps all of its bits, and attributes are untouched.  With finite
float32 inputs no intermediate value can overflow (a difference is below 2^129, a squared length below 2^260, a weight is in [0, 1]
and a sweep moves a joint by at most twice its distance to a weighted mean of its neighbours), so no further non-finite rule is needed.

Known limits.  Spacing after smoothing is no longer exactly uniform, and strands are not resampled again.  lambda|mu amplifies the
lowest frequencies slightly; for very short strands this is visible (a 5-joint arc bends further), and the defaults are knobs, not
measured optima.  There is no feature preservation (curls below the pass band are smoothed like noise) and no strand-to-strand
awareness.  Strands longer than 1024 joints are left alone and counted.

device=None: numpy, vectorised over the strands and their joints, with explicit loops over the sweeps.  device="cuda":
hgs_strand_smooth on torch tensors.  The caller chooses; neither falls back to the other."""
import math

import numpy as np

from scene.strand_collide import _check_points, check_offsets, strand_lengths
from scene.strand_export import StrandExport

SMOOTHED, SHORT, LONG, NONFINITE = range(4)
MAX_JOINTS, MAX_ITERS = 1024, 256


def check_parameters(iters=10, lam=0.5, mu=-0.53, max_move=None):
    """(iters int, lam float, mu float, max_move float or None) of the contract, or ValueError."""
    if isinstance(iters, bool) or int(iters) != iters or not 1 <= int(iters) <= MAX_ITERS:
        raise ValueError(f"iters = {iters}: 1 to {MAX_ITERS}")
    lam, mu = float(lam), float(mu)
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"lam = {lam}: above 0, at most 1")
    if not (mu == 0.0 or -1.0 <= mu < -lam):
        raise ValueError(f"mu = {mu}: 0 (plain Laplacian smoothing), or from -1 to below -lam = {-lam}")
    if not abs((1.0 - 2.0 * lam) * (1.0 - 2.0 * mu)) <= 1.0:
        raise ValueError(f"lam = {lam} with mu = {mu}: |(1 - 2 lam)(1 - 2 mu)| = {abs((1.0 - 2.0 * lam) * (1.0 - 2.0 * mu)):g} is above 1, "
                         "the shortest waves would grow")
    if max_move is not None:
        max_move = float(max_move)
        if not (math.isfinite(max_move) and max_move > 0.0):
            raise ValueError(f"max_move = {max_move}: a finite distance > 0, or None")
    return int(iters), lam, mu, max_move


def longest_eligible(offsets):
    """The number of joints of the longest strand that is neither SHORT nor LONG (0 where there is none): what sizes the kernel's LDS."""
    off = np.asarray(offsets, np.int64)
    n = off[1:] - off[:-1]
    n = n[(n >= 3) & (n <= MAX_JOINTS)]
    return int(n.max()) if n.shape[0] else 0


# ---- numpy path ------------------------------------------------------------------------------------------------------------------
def _ranges(starts, sizes):
    """The concatenation of arange(starts[k], starts[k] + sizes[k])."""
    sizes = np.asarray(sizes, np.int64)
    first = np.cumsum(sizes) - sizes
    return np.repeat(np.asarray(starts, np.int64) - first, sizes) + np.arange(int(sizes.sum()), dtype=np.int64)


def _norm(u):
    return np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])


def smooth_numpy(points, offsets, iters=10, lam=0.5, mu=-0.53, max_move=None):
    """(out_points float32 [P, 3], status int32 [K], clamped int32 [K]) of the contract."""
    points = _check_points(points)
    off = check_offsets(offsets, points.shape[0])
    iters, lam, mu, max_move = check_parameters(iters, lam, mu, max_move)
    K = off.shape[0] - 1
    out = points.copy()
    status, clamped = np.zeros(K, np.int32), np.zeros(K, np.int32)
    n = off[1:] - off[:-1]
    bad = np.concatenate([[0], np.cumsum(~np.isfinite(points).all(axis=1))])      # points that are not finite, in front of each row
    status[(bad[off[1:]] - bad[off[:-1]]) > 0] = NONFINITE
    status[n > MAX_JOINTS] = LONG
    status[n < 3] = SHORT
    S = np.nonzero(status == SMOOTHED)[0]
    if S.size == 0:
        return out, status, clamped
    # the joints of the strands that are smoothed, one after the other: x [Q, 3]; the sweeps work on the rows 1 .. Q - 2 and keep
    # every strand's two end joints
    m = n[S]
    rows = _ranges(off[S], m)
    first = np.cumsum(m) - m
    inner = np.ones(rows.shape[0], bool)
    inner[first], inner[first + m - 1] = False, False
    mid = inner[1:-1, None]
    p = points[rows].astype(np.float64)
    with np.errstate(all="ignore"):                                                # (the rows between two strands are computed and dropped)
        seg = _norm(p[1:] - p[:-1])                                                # seg[i]: from row i to row i + 1
        lm, lc = seg[:-1], seg[1:]                                                 # l_{j-1} and l_j of the rows j = 1 .. Q - 2
        s = lm + lc
        a = np.where(s > 0.0, lc / s, 0.5)[:, None]
        b = np.where(s > 0.0, lm / s, 0.5)[:, None]
        x = p.copy()
        for _ in range(iters):
            for f in (lam, mu):
                if f == 0.0:
                    continue
                xc = x[1:-1]
                new = xc + f * ((a * x[:-2] + b * x[2:]) - xc)                     # sweep t's joints only: `new` is a fresh array
                x[1:-1] = np.where(mid, new, xc)
        if max_move is not None:
            u = x - p
            du = _norm(u)
            hit = inner & (du > max_move)
            x = np.where(hit[:, None], p + (max_move / du)[:, None] * u, x)
            clamped[S] = np.bincount(np.repeat(np.arange(S.size), m)[hit], minlength=S.size).astype(np.int32)
        out[rows[inner]] = x[inner].astype(np.float32)
    return out, status, clamped


# ---- device path -----------------------------------------------------------------------------------------------------------------
def smooth_device(points, offsets, iters=10, lam=0.5, mu=-0.53, max_move=None, max_joints=None):
    """hgs_strand_smooth on device tensors (points float32 [P, 3], offsets int64 [K + 1], already checked: check_offsets): (out_points,
    status, clamped) on the device.  max_joints: longest_eligible(offsets) where the caller has the offsets on the host; None reads
    it off the device tensor (a synchronisation)."""
    import torch
    import hgs_runtime as rt
    points = rt.require_gpu_tensor(points, "points", torch.float32)
    offsets = rt.require_gpu_tensor(offsets, "offsets", torch.int64)
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise rt.HgsError(f"smooth_device: points {tuple(points.shape)} and offsets {tuple(offsets.shape)}; [P, 3] and [K + 1] expected")
    try:
        iters, lam, mu, max_move = check_parameters(iters, lam, mu, max_move)
    except ValueError as e:
        raise rt.HgsError(f"smooth_device: {e}") from None
    P, K, dev = int(points.shape[0]), int(offsets.shape[0]) - 1, points.device
    if max_joints is None:
        n = offsets[1:] - offsets[:-1]
        n = n[(n >= 3) & (n <= MAX_JOINTS)]
        max_joints = int(n.max()) if n.numel() else 0
    if not 0 <= int(max_joints) <= MAX_JOINTS:
        raise rt.HgsError(f"smooth_device: max_joints = {max_joints} (0 to {MAX_JOINTS})")
    out = torch.empty((P, 3), dtype=torch.float32, device=dev)
    status = torch.zeros(K, dtype=torch.int32, device=dev)
    clamped = torch.zeros(K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_strand_smooth(rt.current_stream(), K, rt.ptr(offsets), P, rt.ptr(points), int(max_joints), iters, lam, mu,
                                            int(max_move is not None), 0.0 if max_move is None else max_move, rt.ptr(out), rt.ptr(status),
                                            rt.ptr(clamped)))
    return out, status, clamped


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def mean_turning_angle(points, offsets, strands):
    """The mean angle, in degrees, between the two segments at an inner joint, over the inner joints of the strands `strands` (indices)
    whose two segments both have a finite length > 0; 0.0 where there is none.  float64 on the float32 points."""
    off = np.asarray(offsets, np.int64)
    n = (off[1:] - off[:-1])[strands]
    keep = n >= 3
    j = _ranges(off[strands][keep] + 1, n[keep] - 2)                                # the inner joints' rows
    if j.shape[0] == 0:
        return 0.0
    p = points.astype(np.float64)
    with np.errstate(all="ignore"):
        e0, e1 = p[j] - p[j - 1], p[j + 1] - p[j]
        l0, l1 = _norm(e0), _norm(e1)
        ok = np.isfinite(l0) & np.isfinite(l1) & (l0 > 0.0) & (l1 > 0.0)
        c = ((e0[:, 0] * e1[:, 0] + e0[:, 1] * e1[:, 1]) + e0[:, 2] * e1[:, 2])[ok] / (l0[ok] * l1[ok])
        angle = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
    return float(angle.mean()) if angle.shape[0] else 0.0


def report_of(points, out, offsets, status, clamped):
    """The report of smooth_strands from the host arrays of either path: one set of numpy statements for both."""
    off = np.asarray(offsets, np.int64)
    K = off.shape[0] - 1
    n = off[1:] - off[:-1]
    S = np.nonzero(status == SMOOTHED)[0]
    tally = np.bincount(status, minlength=4)
    inner = _ranges(off[S] + 1, n[S] - 2)
    step = out[inner].astype(np.float64) - points[inner].astype(np.float64)
    disp = _norm(step)
    with np.errstate(all="ignore"):
        before, after = strand_lengths(points, off)[S], strand_lengths(out, off)[S]
        ratio = (after / before)[before > 0.0]
    return dict(strands=K, smoothed=int(tally[SMOOTHED]), short=int(tally[SHORT]), long=int(tally[LONG]), nonfinite=int(tally[NONFINITE]),
                joints=int(points.shape[0]), clamped=int(clamped.sum(dtype=np.int64)),
                largest_displacement=float(disp.max()) if disp.shape[0] else 0.0,
                mean_displacement=float(disp.mean()) if disp.shape[0] else 0.0,
                turning_before=mean_turning_angle(points, off, S), turning_after=mean_turning_angle(out, off, S),
                length_ratio_min=float(ratio.min()) if ratio.shape[0] else 1.0,
                length_ratio_mean=float(ratio.mean()) if ratio.shape[0] else 1.0,
                length_ratio_max=float(ratio.max()) if ratio.shape[0] else 1.0)


def smooth_strands(strands, iters=10, lam=0.5, mu=-0.53, max_move=None, device=None):
    """`strands` (a StrandExport, ragged or not) low-passed, see the module docstring: (StrandExport, report).  report: "strands",
    "smoothed", "short", "long", "nonfinite" (strands by status), "joints", "clamped" (joints held at max_move), "largest_displacement"
    and "mean_displacement" (over the inner joints of the smoothed strands), "turning_before" and "turning_after" (the mean turning
    angle per inner joint of the smoothed strands, degrees) and "length_ratio_min", "length_ratio_mean", "length_ratio_max" (a smoothed
    strand's length after over its length before).  device=None: numpy; "cuda": the HIP kernel."""
    points = _check_points(strands.points)
    off = check_offsets(strands.offsets, points.shape[0])
    iters, lam, mu, max_move = check_parameters(iters, lam, mu, max_move)
    if device is None:
        out, status, clamped = smooth_numpy(points, off, iters, lam, mu, max_move)
    else:
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernel)")
        import torch
        res = smooth_device(torch.as_tensor(points, device=device), torch.as_tensor(off, device=device), iters, lam, mu, max_move,
                            max_joints=longest_eligible(off))
        out, status, clamped = (t.cpu().numpy() for t in res)
    report = report_of(points, out, off, status, clamped)
    return StrandExport(out, strands.attrs, strands.offsets, strands.strand_ids, strand_lengths(out, off)), report
