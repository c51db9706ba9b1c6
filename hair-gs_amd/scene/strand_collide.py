"""Exported strands pushed out of the head, keeping their segment lengths (export_strands.py --resolve_head): a blended strand
(scene/groom.py) cuts through the head near the ears, the nape and a parting, and a trained one can carry sunk joints (--lambda_head
is off by default).  Every strand is walked from its root; a joint inside the head is pushed out along the gradient of the capture's
distance field (utils/head_sdf.py), and every joint behind it follows the leader: it aims at its original place and stays a segment's
length from its moved predecessor, so the strand returns to its trained path behind the obstacle.

The contract (this module's numpy path, csrc/hgs_collide.hip and the loop restatement in tests/collide_reference.py state the same
thing).  All strand arithmetic is float64 with one rounding per operation, in exactly the order written, and dot(u, v) = (u0*v0 +
u1*v1) + u2*v2.  The field is sampled by the float32 Term statement of utils/head_sdf.py (the kernel file is built with
-ffp-contract=off).

Inputs.  points float32 [P, 3].  offsets int64 [K + 1] with offsets[0] == 0, non-decreasing, offsets[K] == P (Python checks this; the
kernel trusts it).  A HeadSDF: phi float32 [nz, ny, nx], origin32, inv_h32, at least 2 nodes an axis.  margin float32, finite, >= 0.
skin float32, finite, >= 0; the default is float32(1e-3 * spacing): it puts a pushed joint just past the margin, so that rounding to
float32 does not leave it a few ulps inside.  iters 1..32, default 8.

Sampling, S(x) for a float64 x.  p = float32(x) per coordinate; then exactly the Term statement of utils/head_sdf.py: t, "in range",
d, gx, gy, gz, in float32.  It returns (ok, d, g).  A point that is not finite, or out of range, has ok false and counts as outside.

Per strand s (joints a .. a + n - 1).  A strand with n < 2 is copied.
    q_0 = (double)p_0: the root never moves, even when it is inside the margin.  moved = false.
    For j = 1 .. n - 1:
        e = (double)p_j - (double)p_{j-1} on the ORIGINAL points; L = sqrt(dot(e, e)).
        relen(x):  u = x - q_{j-1}; lu = sqrt(dot(u, u)).  If L is finite and lu is finite and > 0: f = L / lu and the result is
                   q_{j-1} + f*u per coordinate.  Otherwise the result is q_{j-1} + e.
        x = (double)p_j.  If moved: x = relen(x)  (follow the leader).
        hit = false.  Repeat at most `iters` times:
            (ok, d, g) = S(x).  Stop unless ok and d < margin.
            G = (double)g; gn = sqrt(dot(G, G)).  Stop unless gn is finite and > 0.
            x = x + ((((double)margin + (double)skin) - (double)d) / gn) * G per coordinate.
            hit = true.
            x = relen(x).
        If hit: moved = true and moved_count[s] += 1.
        q_j = x; out_j = float32(q_j).
        (ok, d, _) = S(q_j).  If ok and d < margin: unresolved[s] += 1.

Consequences.  Every joint up to a strand's first hit keeps its bits, a strand that never penetrates keeps all of them, and segment
lengths are those of the input up to the float32 rounding of the output points.

Outputs.  out_points float32 [P, 3], moved int32 [K], unresolved int32 [K].  Attributes are untouched; resolve_head recomputes `length`
by scene.groom.polyline_length's statement on the output (per strand, ragged), one statement for both paths.

Known limits.  Only joints are tested: a long segment can still cut a corner.  There is no strand-to-strand collision.  A joint where
the gradient vanishes stays inside and is counted as unresolved; so is a joint that a root inside the head (which never moves) holds
inside at its segment's length, and one that `iters` pushes did not bring out.

device=None: numpy, vectorised over the strands, with explicit loops over the joints and the pushes so that the order of operations is
the one above.  device="cuda": hgs_strand_collide on torch tensors.  The caller chooses; neither falls back to the other."""

import numpy as np

from scene.strand_export import StrandExport
from utils import head_sdf

MAX_ITERS = 32


def default_skin(sdf):
    return np.float32(1e-3 * sdf.spacing)


def check_parameters(sdf, margin, skin, iters):
    """(margin float32, skin float32, iters int) of the contract, or ValueError."""
    if min(sdf.shape) < 2:
        raise ValueError(f"a field of {sdf.shape} nodes: at least 2 an axis")
    margin = np.float32(margin)
    skin = default_skin(sdf) if skin is None else np.float32(skin)
    if not (np.isfinite(margin) and margin >= 0):
        raise ValueError(f"margin = {margin}: finite and >= 0")
    if not (np.isfinite(skin) and skin >= 0):
        raise ValueError(f"skin = {skin}: finite and >= 0")
    if int(iters) != iters or not 1 <= int(iters) <= MAX_ITERS:
        raise ValueError(f"iters = {iters}: 1 to {MAX_ITERS}")
    return margin, skin, int(iters)


def check_offsets(offsets, P):
    """offsets as a contiguous int64 [K + 1] array whose ranges tile the P points, or ValueError."""
    off = np.asarray(offsets)
    if off.ndim != 1 or off.shape[0] < 1 or off.dtype.kind not in "iu":
        raise ValueError(f"offsets of shape {off.shape} and type {off.dtype}: an integer array [K + 1] expected")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off[0] != 0 or off[-1] != P or np.any(off[1:] < off[:-1]):
        raise ValueError(f"offsets must start at 0, not decrease and end at the number of points ({P})")
    return off


def _check_points(points):
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points of shape {points.shape}: [P, 3] expected")
    return np.ascontiguousarray(points, dtype=np.float32)


# ---- numpy path ------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sample(x, sdf):
    """S(x) of the contract for float64 coordinate columns x = [x0, x1, x2]: (ok, d, [gx, gy, gz])."""
    ok, d, gx, gy, gz = head_sdf.trilinear(np.stack(x, axis=1).astype(np.float32), sdf)
    return ok, d, [gx, gy, gz]


def _relen(x, q, e, L):
    u = [x[c] - q[c] for c in range(3)]
    lu = np.sqrt(_dot(u, u))
    good = np.isfinite(L) & np.isfinite(lu) & (lu > 0.0)
    f = L / lu
    return [np.where(good, q[c] + f * u[c], q[c] + e[c]) for c in range(3)]


def resolve_numpy(points, offsets, sdf, margin=0.0, skin=None, iters=8):
    """(out_points float32 [P, 3], moved int32 [K], unresolved int32 [K]) of the contract."""
    points = _check_points(points)
    off = check_offsets(offsets, points.shape[0])
    margin, skin, iters = check_parameters(sdf, margin, skin, iters)
    K = off.shape[0] - 1
    out = points.copy()
    moved_count, unresolved = np.zeros(K, np.int32), np.zeros(K, np.int32)
    n = off[1:] - off[:-1]
    if K == 0 or n.max() < 2:
        return out, moved_count, unresolved
    reach = np.float64(margin) + np.float64(skin)
    strands = np.nonzero(n >= 2)[0]                                         # the strands still being walked, ascending
    q = [points[off[strands], c].astype(np.float64) for c in range(3)]       # q_{j-1} of each
    moved = np.zeros(strands.shape[0], bool)
    with np.errstate(all="ignore"):
        for j in range(1, int(n.max())):
            keep = n[strands] > j
            if not keep.all():
                strands, moved, q = strands[keep], moved[keep], [v[keep] for v in q]
            row = off[strands] + j
            pj = [points[row, c].astype(np.float64) for c in range(3)]
            e = [pj[c] - points[row - 1, c].astype(np.float64) for c in range(3)]
            L = np.sqrt(_dot(e, e))
            led = _relen(pj, q, e, L)
            x = [np.where(moved, led[c], pj[c]) for c in range(3)]
            hit = np.zeros(strands.shape[0], bool)
            live = np.arange(strands.shape[0])                               # rows whose push loop has not stopped
            for _ in range(iters):
                if live.size == 0:
                    break
                xs = [v[live] for v in x]
                ok, d, g = _sample(xs, sdf)
                G = [v.astype(np.float64) for v in g]
                gn = np.sqrt(_dot(G, G))
                go = ok & (d < margin) & np.isfinite(gn) & (gn > 0.0)
                live = live[go]
                if live.size == 0:
                    break
                step = (reach - d[go].astype(np.float64)) / gn[go]
                xs = [xs[c][go] + step * G[c][go] for c in range(3)]
                xs = _relen(xs, [v[live] for v in q], [v[live] for v in e], L[live])
                for c in range(3):
                    x[c][live] = xs[c]
                hit[live] = True
            moved |= hit
            moved_count[strands] += hit.astype(np.int32)
            for c in range(3):
                out[row, c] = x[c].astype(np.float32)
            ok, d, _ = _sample(x, sdf)
            unresolved[strands] += (ok & (d < margin)).astype(np.int32)
            q = x
    return out, moved_count, unresolved


# ---- device path -----------------------------------------------------------------------------------------------------------------
def resolve_device(points, offsets, sdf, margin=0.0, skin=None, iters=8):
    """hgs_strand_collide on device tensors (points float32 [P, 3], offsets int64 [K + 1], already checked: check_offsets): (out_points,
    moved, unresolved) on the device.  The field's device copy is the HeadSDF's cached one."""
    import torch
    import hgs_runtime as rt
    points = rt.require_gpu_tensor(points, "points", torch.float32)
    offsets = rt.require_gpu_tensor(offsets, "offsets", torch.int64)
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise rt.HgsError(f"resolve_device: points {tuple(points.shape)} and offsets {tuple(offsets.shape)}; [P, 3] and [K + 1] expected")
    try:
        margin, skin, iters = check_parameters(sdf, margin, skin, iters)
    except ValueError as e:
        raise rt.HgsError(f"resolve_device: {e}") from None
    P, K, dev = int(points.shape[0]), int(offsets.shape[0]) - 1, points.device
    field = sdf.on(dev)
    nx, ny, nz = sdf.shape
    if field["phi"].numel() != nx * ny * nz:
        raise rt.HgsError(f"resolve_device: a field of {field['phi'].numel()} values for a grid of {nx} x {ny} x {nz} nodes")
    out = torch.empty((P, 3), dtype=torch.float32, device=dev)
    moved = torch.zeros(K, dtype=torch.int32, device=dev)
    unresolved = torch.zeros(K, dtype=torch.int32, device=dev)
    o = sdf.origin32
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_strand_collide(rt.current_stream(), K, rt.ptr(offsets), P, rt.ptr(points), rt.ptr(field["phi"]), nx, ny, nz,
                                             float(o[0]), float(o[1]), float(o[2]), float(sdf.inv_h32), float(margin), float(skin), iters,
                                             rt.ptr(out), rt.ptr(moved), rt.ptr(unresolved)))
    return out, moved, unresolved


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def strand_lengths(points, offsets):
    """float64 [K]: scene.groom.polyline_length's statement for ragged strands -- the float64 segment lengths of the float32 points,
    added up in segment order per strand; 0 for a strand without a segment."""
    off = np.asarray(offsets, np.int64)
    K, P = off.shape[0] - 1, points.shape[0]
    length = np.zeros(K, np.float64)
    if P < 2:
        return length
    p = points.astype(np.float64)
    d = p[1:] - p[:-1]
    seg = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])     # seg[i]: from point i to i + 1
    n = off[1:] - off[:-1]
    for m in np.unique(n[n >= 2]):                                                   # strands of one size at a time: a cumsum each
        s = np.nonzero(n == m)[0]
        rows = off[s][:, None] + np.arange(m - 1)[None, :]
        length[s] = np.cumsum(seg[rows], axis=1)[:, -1]
    return length


def _inside(d, margin):
    """(count, deepest) of the distances d (float32, +inf out of range): joints with d < margin, and the largest margin - d."""
    hit = d[d < margin]
    return int(hit.shape[0]), (float(np.float64(margin) - np.float64(hit.min())) if hit.shape[0] else 0.0)


def resolve_head(strands, sdf, margin=0.0, iters=8, skin=None, device=None):
    """`strands` (a StrandExport, ragged or not) pushed out of the head of `sdf` (a HeadSDF), see the module docstring: (StrandExport,
    stats).  stats: "joints", "inside_before", "inside_after" (joints in range with d < margin, roots included), "deepest_before",
    "deepest_after" (the largest margin - d of those, 0 where there is none), "moved" (joints pushed), "unresolved" (joints behind a
    root left with d < margin), "strands_touched" and "largest_displacement".  device=None: numpy; "cuda": the HIP kernel."""
    points = _check_points(strands.points)
    off = check_offsets(strands.offsets, points.shape[0])
    margin, skin, iters = check_parameters(sdf, margin, skin, iters)
    if device is None:
        out, moved, unresolved = resolve_numpy(points, off, sdf, margin, skin, iters)
        with np.errstate(all="ignore"):
            d0, d1 = (np.where(ok, d, np.float32(np.inf)) for ok, d, _, _, _ in (head_sdf.trilinear(points, sdf), head_sdf.trilinear(out, sdf)))
    else:
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernel)")
        import torch
        from hgs_runtime.fused import head_penalty
        pts_d, off_d = torch.as_tensor(points, device=device), torch.as_tensor(off, device=device)
        out_d, moved_d, unresolved_d = resolve_device(pts_d, off_d, sdf, margin, skin, iters)
        info = {}
        dist = []
        for t in (pts_d, out_d):                                               # (the scratch is the call's own: "dist" is a fresh tensor)
            head_penalty(t, sdf, float(margin), info)
            dist.append(info["dist"].cpu().numpy())
        d0, d1 = dist
        out, moved, unresolved = out_d.cpu().numpy(), moved_d.cpu().numpy(), unresolved_d.cpu().numpy()
    with np.errstate(all="ignore"):
        before, after = _inside(d0, margin), _inside(d1, margin)
        step = out.astype(np.float64) - points.astype(np.float64)
        disp = np.sqrt((step[:, 0] * step[:, 0] + step[:, 1] * step[:, 1]) + step[:, 2] * step[:, 2])
        disp = disp[np.isfinite(disp)]
        length = strand_lengths(out, off)
    stats = dict(joints=int(points.shape[0]), inside_before=before[0], inside_after=after[0], deepest_before=before[1],
                 deepest_after=after[1], moved=int(moved.sum(dtype=np.int64)), unresolved=int(unresolved.sum(dtype=np.int64)),
                 strands_touched=int(np.count_nonzero(moved)), largest_displacement=float(disp.max()) if disp.shape[0] else 0.0)
    return StrandExport(out, strands.attrs, strands.offsets, strands.strand_ids, length), stats
