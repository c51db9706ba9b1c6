"""Exported strands simplified to a tolerance (export_strands.py --simplify TOL): every step of the export chain keeps a strand's point
count or multiplies it, and the interchange form is --points M for all strands, so a straight strand costs what a curl costs.  The
formats the tool writes are ragged by design (.hair has a segment count per strand, .data a point count, the PLYs an edge list).  This
is the last step in front of the writers: every joint that lies within `tol` of the chord that replaces it is dropped, so each strand
keeps as many joints as its shape needs.  The rule is Douglas-Peucker's with the distance to the SEGMENT, not to the line, so a curl
that turns back over its chord is not flattened.

The contract (this module's numpy path, csrc/hgs_strand_simplify.hip and the recursive restatement in tests/simplify_reference.py
state the same thing).  It follows scene/strand_collide.py's and scene/strand_smooth.py's conventions: strands are ragged; all
arithmetic is float64 on the float32 inputs, with one rounding per operation, in exactly the order written; dot(u, v) =
(u0*v0 + u1*v1) + u2*v2 (the kernel file is built with -ffp-contract=off).

Inputs.  points float32 [P, 3].  offsets int64 [K + 1] (strand_collide.check_offsets).  tol float64.

Parameter check (check_parameters raises ValueError; the device wrapper raises HgsError).  tol is finite and >= 0.

Per strand s with joints p_0 .. p_{n-1} as float64:
    status SHORT (1): n < 3.  LONG (2): n > MAX_JOINTS = 1024, or, on the device, n > the launch's max_joints (its LDS slice).
    NONFINITE (3): any coordinate is not finite.  Every joint of such a strand is kept, and rounds[s] = 0.  Otherwise OK (0):
    Deviation d2(p; a, b) of a joint p from the interval with the end joints a, b:
        ab = b - a;  ap = p - a;  L2 = dot(ab, ab);  t = dot(ap, ab) / L2 where L2 > 0, else 0;  t < 0 becomes 0, t > 1 becomes 1;
        q_c = ap_c - t*ab_c per component;  d2 = dot(q, q).
    Selection.  tol2 = tol*tol, formed once.  keep[0] = keep[n-1] = 1.  The interval (0, n-1) has depth 1.  For an interval (i, k) of
        consecutive kept joints with k > i + 1, j* is the joint of i < j < k with the largest d2(p_j; p_i, p_k), the smallest such j
        where several are equal.  If d2(j*) > tol2 (strict), j* is kept and the intervals (i, j*) and (j*, k), of the next depth, are
        treated the same way.  Otherwise every joint between i and k is dropped.
    rounds[s] is the largest depth at which a joint was kept (0 where none was).
    The intervals of one depth are independent of each other, and an interval's treatment depends on nothing but its two end joints,
    so "all the intervals of a depth at once" (the kernel, the numpy path) keeps the joints the recursion keeps in any order.

Outputs.  keep uint8 [P] (1: kept), status int32 [K], rounds int32 [K].  The simplified strands are the kept joints in order with the
input bits of their points and attributes -- nothing is interpolated or rounded --, offsets the prefix sums of the kept counts,
strand_ids unchanged and length recomputed by strand_collide.strand_lengths.

Consequences.  Every dropped joint lies within tol of the segment that replaced it (its d2 against that segment, by the statement
above, is <= tol2: it was compared with exactly that segment when its interval was closed).  Roots and tips keep their bits.  tol = 0
drops only joints with d2 == 0 (joints on their segment).  The result is idempotent: simplifying the output with the same tol makes
the same splits again (an interval's winner is among the kept joints, still its largest and its first) and closes only intervals
without a joint between, so it keeps every joint and takes the same rounds.  With finite float32 inputs no intermediate value overflows or is a NaN (a difference is below 2^129, a squared length below 2^260
and above 2^-299 where it is not 0, t is in [0, 1]), so no further non-finite rule is needed.

Known limits.  The rule is geometry only: attributes between kept joints become linear in a consumer, and the report says by how much
they were not.  It is not the minimum-joint solution for the tolerance.  There is no awareness of neighbouring strands (two strands
that did not cross may cross by less than 2 tol).  Strands longer than 1024 joints are left alone and counted.

device=None: numpy, vectorised over all strands, one pass per depth.  device="cuda": hgs_strand_simplify on torch tensors.  The
caller chooses; neither falls back to the other."""
import math

import numpy as np

from scene.strand_collide import _check_points, check_offsets, strand_lengths
from scene.strand_export import StrandExport
from scene.strand_smooth import _ranges, longest_eligible

OK, SHORT, LONG, NONFINITE = range(4)
MAX_JOINTS = 1024


def check_parameters(tol):
    """tol of the contract as a float, or ValueError."""
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"tol = {tol!r}: a finite distance >= 0") from None
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"tol = {tol}: a finite distance >= 0")
    return tol


# ---- numpy path ------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def deviation(p, a, b):
    """(d2, t) of the contract for rows of float64 joints p against the intervals with the end joints a, b."""
    ab, ap = b - a, p - a
    L2 = _dot(ab, ab)
    with np.errstate(all="ignore"):
        t = np.where(L2 > 0.0, _dot(ap, ab) / L2, 0.0)
    t = np.where(t < 0.0, 0.0, t)
    t = np.where(t > 1.0, 1.0, t)
    q = ap - t[:, None] * ab
    return _dot(q, q), t


def _neighbours(kept):
    """(lo, hi): for every row the nearest kept row at or below it and at or above it (the rows' strands begin and end kept)."""
    idx = np.arange(kept.shape[0], dtype=np.int64)
    lo = np.maximum.accumulate(np.where(kept, idx, -1))
    hi = np.minimum.accumulate(np.where(kept, idx, kept.shape[0])[::-1])[::-1]
    return lo, hi


def strand_status(points, off):
    """status int32 [K] of the contract (the host's: LONG is n > MAX_JOINTS)."""
    n = off[1:] - off[:-1]
    status = np.zeros(n.shape[0], np.int32)
    bad = np.concatenate([[0], np.cumsum(~np.isfinite(points).all(axis=1))])      # points that are not finite, in front of each row
    status[(bad[off[1:]] - bad[off[:-1]]) > 0] = NONFINITE
    status[n > MAX_JOINTS] = LONG
    status[n < 3] = SHORT
    return status


def simplify_numpy(points, offsets, tol):
    """(keep uint8 [P], status int32 [K], rounds int32 [K]) of the contract."""
    points = _check_points(points)
    off = check_offsets(offsets, points.shape[0])
    tol = check_parameters(tol)
    K = off.shape[0] - 1
    keep = np.ones(points.shape[0], np.uint8)
    status, rounds = strand_status(points, off), np.zeros(K, np.int32)
    S = np.nonzero(status == OK)[0]
    if S.size == 0:
        return keep, status, rounds
    # the joints of the OK strands, one strand after the other: x [Q, 3]
    m = (off[1:] - off[:-1])[S]
    rows = _ranges(off[S], m)
    first = np.cumsum(m) - m
    strand_of = np.repeat(S, m)
    x = points[rows].astype(np.float64)
    Q = rows.shape[0]
    kept = np.zeros(Q, bool)
    kept[first], kept[first + m - 1] = True, True
    tol2 = tol * tol
    live = np.nonzero(~kept)[0]                                                     # the joints of intervals that are still open
    depth = 0
    while live.size:
        depth += 1
        lo, hi = _neighbours(kept)
        i = lo[live]
        d2, _ = deviation(x[live], x[i], x[hi[live]])
        cand = d2 > tol2
        j, i, d2 = live[cand], i[cand], d2[cand]
        if j.size == 0:
            break
        order = np.lexsort((j, -d2, i))                                             # by interval, then d2 falling, then j rising
        i = i[order]
        head = np.ones(i.shape[0], bool)
        head[1:] = i[1:] != i[:-1]
        win = j[order][head]
        kept[win] = True
        rounds[strand_of[win]] = depth
        split = np.zeros(Q, bool)                                                   # by an interval's left end: it kept a joint
        split[i[head]] = True
        live = live[split[lo[live]] & ~kept[live]]
    keep[rows] = kept
    return keep, status, rounds


# ---- device path -----------------------------------------------------------------------------------------------------------------
def simplify_device(points, offsets, tol, max_joints=None):
    """hgs_strand_simplify on device tensors (points float32 [P, 3], offsets int64 [K + 1], already checked: check_offsets): (keep
    uint8 [P], status int32 [K], rounds int32 [K]) on the device.  max_joints: longest_eligible(offsets) where the caller has the
    offsets on the host; None reads it off the device tensor (a synchronisation).  A strand longer than max_joints is LONG."""
    import torch
    import hgs_runtime as rt
    points = rt.require_gpu_tensor(points, "points", torch.float32)
    offsets = rt.require_gpu_tensor(offsets, "offsets", torch.int64)
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise rt.HgsError(f"simplify_device: points {tuple(points.shape)} and offsets {tuple(offsets.shape)}; [P, 3] and [K + 1] expected")
    try:
        tol = check_parameters(tol)
    except ValueError as e:
        raise rt.HgsError(f"simplify_device: {e}") from None
    P, K, dev = int(points.shape[0]), int(offsets.shape[0]) - 1, points.device
    if max_joints is None:
        n = offsets[1:] - offsets[:-1]
        n = n[(n >= 3) & (n <= MAX_JOINTS)]
        max_joints = int(n.max()) if n.numel() else 0
    if int(max_joints) != 0 and not 3 <= int(max_joints) <= MAX_JOINTS:
        raise rt.HgsError(f"simplify_device: max_joints = {max_joints} (3 to {MAX_JOINTS}, or 0 where no strand is eligible)")
    keep = torch.empty(P, dtype=torch.uint8, device=dev)
    status = torch.zeros(K, dtype=torch.int32, device=dev)
    rounds = torch.zeros(K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_strand_simplify(rt.current_stream(), K, rt.ptr(offsets), P, rt.ptr(points), int(max_joints), tol,
                                              rt.ptr(keep), rt.ptr(status), rt.ptr(rounds)))
    return keep, status, rounds


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def take_strands(strands, index):
    """The StrandExport of the strands index [G] names, in index's order (ragged or not), every bit kept."""
    off = np.asarray(strands.offsets, np.int64)
    index = np.asarray(index, np.int64)
    n = (off[1:] - off[:-1])[index]
    rows = _ranges(off[index], n)
    return StrandExport(np.asarray(strands.points)[rows], np.asarray(strands.attrs)[rows], np.concatenate([[0], np.cumsum(n)]).astype(np.int64),
                        np.asarray(strands.strand_ids)[index], np.asarray(strands.length)[index])


def report_of(points, attrs, offsets, keep, status, rounds):
    """The report of simplify_strands from the host arrays of either path: one set of numpy statements for both."""
    off = np.asarray(offsets, np.int64)
    K, P = off.shape[0] - 1, points.shape[0]
    kept = keep != 0
    tally = np.bincount(status, minlength=4)
    c = np.concatenate([[0], np.cumsum(kept)])
    count = (c[off[1:]] - c[off[:-1]])[status == OK]
    after = int(c[-1])
    attrs = np.asarray(attrs).reshape(P, -1)
    dropped = np.nonzero(~kept)[0]
    largest, attr_dev = 0.0, [0.0] * attrs.shape[1]
    if dropped.shape[0]:
        lo, hi = _neighbours(kept)
        i, k = lo[dropped], hi[dropped]
        x = points.astype(np.float64)
        d2, t = deviation(x[dropped], x[i], x[k])
        largest = float(np.sqrt(d2.max()))
        a = attrs.astype(np.float64)
        linear = a[i] + t[:, None] * (a[k] - a[i])
        attr_dev = [float(v) for v in np.abs(a[dropped] - linear).max(axis=0)]
    return dict(strands=K, ok=int(tally[OK]), short=int(tally[SHORT]), long=int(tally[LONG]), nonfinite=int(tally[NONFINITE]),
                joints_before=int(P), joints_after=after, ratio=float(after) / float(P) if P else 1.0,
                kept_min=int(count.min()) if count.shape[0] else 0, kept_mean=float(count.mean()) if count.shape[0] else 0.0,
                kept_max=int(count.max()) if count.shape[0] else 0, rounds_max=int(rounds.max()) if K else 0,
                largest_deviation=largest, attr_deviation=attr_dev)


def simplify_strands(strands, tol, device=None):
    """`strands` (a StrandExport, ragged or not) simplified to `tol`, see the module docstring: (StrandExport, report).  report:
    "strands", "ok", "short", "long", "nonfinite" (strands by status), "joints_before", "joints_after", "ratio" (after / before),
    "kept_min", "kept_mean", "kept_max" (the kept joints of an OK strand), "rounds_max", "largest_deviation" (of a dropped joint from
    the segment between the kept joints around it, by the contract's statement) and "attr_deviation" (per attribute column, the largest
    difference between a dropped joint's value and the value linear in t between that segment's end joints).  device=None: numpy;
    "cuda": the HIP kernel."""
    points = _check_points(strands.points)
    off = check_offsets(strands.offsets, points.shape[0])
    tol = check_parameters(tol)
    attrs = np.asarray(strands.attrs)
    if device is None:
        keep, status, rounds = simplify_numpy(points, off, tol)
    else:
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernel)")
        import torch
        res = simplify_device(torch.as_tensor(points, device=device), torch.as_tensor(off, device=device), tol, max_joints=longest_eligible(off))
        keep, status, rounds = (t.cpu().numpy() for t in res)
    report = report_of(points, attrs, off, keep, status, rounds)
    kept = keep != 0
    c = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    new_off = np.ascontiguousarray(c[off])
    out = points[kept]
    return StrandExport(out, attrs[kept], new_off, strands.strand_ids, strand_lengths(out, new_off)), report
