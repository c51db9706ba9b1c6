"""A dense groom interpolated from the trained strands (export_strands.py --interpolate): the strands a model trained, resampled to a
fixed number of points (scene/strand_export.py), serve as *guides*, and every root on the scalp gets a strand blended from the guides
rooted nearest to it.

The contract (this path, csrc/hgs_groom.hip and the tests' loop restatement state the same thing).  All arithmetic is float64 on the
given inputs, one rounding per operation; results are rounded once to float32.

Inputs.  Guides: K strands of exactly M >= 2 points, gp float32 [K, M, 3] and ga float32 [K, M, C], 1 <= C <= 16 -- the output of
resample_strands(model, points=M, ...) after its filters (native mode, points=0, has ragged strands and is refused).  Roots: r float64
[N, 3].  Parameters: k guides per root (1..8), max_d2 (a finite value, or +inf for no limit), cos_max.

Per guide g.  Chord c_g = (double)gp[g][M-1] - (double)gp[g][0], len_g = sqrt((cx*cx + cy*cy) + cz*cz).

Search, per root n.  For every guide g in ascending g: dx = r_x - (double)gp[g][0][x], likewise dy and dz; d2 = (dx*dx + dy*dy) + dz*dz.
Candidates with a non-finite d2 or with d2 > max_d2 are skipped (a non-finite root or guide root never matches).  The list is the k
candidates smallest by (d2, g): ties go to the smaller g.

Parting rule (a root between the two sides of a parting must not get the average of two opposite falls).  Rank 0, the nearest guide
g0, is always kept.  A guide at rank i >= 1 is kept iff len_gi > 0 and len_g0 > 0 and (cix*c0x + ciy*c0y) + ciz*c0z >= cos_max *
(len_gi * len_g0).  Dropped guides are removed and the list is compacted in rank order.  cos_max = cos(radians(max_angle)), and -2 for
max_angle >= 180.  If d2 of rank 0 is exactly 0 the list is cut to rank 0 alone.

Weights.  w_i = d2_0 / d2_i (inverse squared distance relative to the nearest: scale-free, no softening constant), w_0 = 1 in both
cases; W = the w_i summed in rank order starting from 0.0; w^_i = w_i / W.

Outputs of the search.  idx int32 [N, k], d2 float64 [N, k], w float64 [N, k] (the normalised w^), count int32 [N]; slots at or past
count hold -1, +inf and 0.  A root with count == 0 is dropped.

Blend, per kept root n, point j (0..M-1), coordinate c.  acc = 0.0; for i = 0..count-1: acc = acc + w^_i * ((double)gp[g_i][j][c] -
(double)gp[g_i][0][c]); point = (float)(r_c + acc).  Attributes: acc = acc + w^_i * (double)ga[g_i][j][a], then (float)acc.  Point 0 of
every strand is its root rounded to float32.

Result.  A StrandExport (points, attrs, uniform offsets of M) with strand_ids = first_id + root number (first_id: the model's number
of strands, so that --colour strand hues stay distinct) and length = the float64 polyline length of the float32 output points, added
up in segment order (one numpy statement for both paths); the kept root numbers (ascending), the number of dropped roots and the
number of guides behind every kept root.

What this does not do: the guides' offsets are not rotated to the local scalp normal, there is no jitter or clumping, and no
collision response of its own -- an interpolated strand can pass through the head.  Pushing such points out is the step behind this
one, scene/strand_collide.py (export_strands.py --resolve_head); without that flag export_strands.py counts them where it has the
capture's distance field and writes them as they are.

device=None: numpy, vectorised over the roots, with explicit loops over the at most 8 ranks so that the sums keep rank order.
device="cuda": hgs_groom_neighbours / hgs_groom_blend on torch tensors, the kept list built by one nonzero between the launches.  The
caller chooses; neither falls back to the other."""
import math
from typing import NamedTuple

import numpy as np
import torch

from scene.strand_export import StrandExport

_BUDGET = 1 << 21          # elements of one vectorised block (roots x guides, or roots x points)


class Groom(NamedTuple):
    strands: StrandExport    # the interpolated strands, one per kept root
    root_ids: np.ndarray     # int64 [n_kept]: numbers of the kept roots, ascending
    n_dropped: int           # roots without a guide in reach
    n_guides: np.ndarray     # int32 [n_kept]: guides blended into every kept root's strand


def search_parameters(max_guide_distance, max_angle):
    """(max_d2, cos_max) of the contract from the user's distance (None: no limit) and angle in degrees."""
    if max_guide_distance is None:
        max_d2 = math.inf
    else:
        D = float(max_guide_distance)
        if not (D >= 0.0) or math.isinf(D):
            raise ValueError(f"max_guide_distance = {max_guide_distance}: a finite distance >= 0, or None for no limit")
        max_d2 = D * D
    a = float(max_angle)
    if not (a >= 0.0):
        raise ValueError(f"max_angle = {max_angle}: degrees >= 0 (180 or more: no parting rule)")
    return max_d2, (-2.0 if a >= 180.0 else math.cos(math.radians(a)))


def _check(gp, ga, roots, k):
    if gp.ndim != 3 or gp.shape[2] != 3 or ga.ndim != 3 or ga.shape[:2] != gp.shape[:2]:
        raise ValueError(f"guides: points {tuple(gp.shape)} and attributes {tuple(ga.shape)}; [K, M, 3] and [K, M, C] expected")
    if gp.shape[1] < 2:
        raise ValueError(f"guides of {gp.shape[1]} points: at least 2 points per guide")
    if not 1 <= ga.shape[2] <= 16:
        raise ValueError(f"guides with {ga.shape[2]} attributes: 1 to 16")
    if roots.ndim != 2 or roots.shape[1] != 3:
        raise ValueError(f"roots of shape {tuple(roots.shape)}: [N, 3] expected")
    if not 1 <= int(k) <= 8:
        raise ValueError(f"k = {k}: 1 to 8 guides per root")


# ---- numpy path ------------------------------------------------------------------------------------------------------------------
def _chords(gp):
    c = gp[:, -1].astype(np.float64) - gp[:, 0].astype(np.float64)
    return c, np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def search_numpy(gp, roots, k, max_d2, cos_max):
    """(idx int32 [N, k], d2 float64 [N, k], w float64 [N, k], count int32 [N]) of the contract."""
    N, K, k = roots.shape[0], gp.shape[0], int(k)
    idx, d2o = np.full((N, k), -1, np.int32), np.full((N, k), np.inf, np.float64)
    wo, count = np.zeros((N, k), np.float64), np.zeros(N, np.int32)
    if N == 0 or K == 0:
        return idx, d2o, wo, count
    g0 = gp[:, 0].astype(np.float64)
    chord, clen = _chords(gp)
    max_d2 = np.float64(max_d2)
    step = max(1, _BUDGET // K)
    with np.errstate(all="ignore"):
        for b in range(0, N, step):
            r = roots[b:b + step]
            B = r.shape[0]
            dx, dy, dz = (r[:, c, None] - g0[None, :, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2[~(np.isfinite(d2) & (d2 <= max_d2))] = np.inf
            rows = np.arange(B)
            cand_g, cand_d = np.empty((B, k), np.int64), np.empty((B, k), np.float64)
            for i in range(min(k, K)):                 # the smallest by (d2, g): argmin names the first of equal values
                g = np.argmin(d2, axis=1)
                cand_g[:, i], cand_d[:, i] = g, d2[rows, g]
                d2[rows, g] = np.inf
            cand_d[:, min(k, K):] = np.inf
            cand_g[:, min(k, K):] = 0
            c0, len0, d0 = chord[cand_g[:, 0]], clen[cand_g[:, 0]], cand_d[:, 0]
            pos = np.zeros(B, np.int64)
            W = np.zeros(B, np.float64)
            wi = np.zeros((B, k), np.float64)
            for i in range(k):
                valid = cand_d[:, i] < np.inf
                if i == 0:
                    keep, w = valid, np.ones(B, np.float64)
                else:
                    ci, leni = chord[cand_g[:, i]], clen[cand_g[:, i]]
                    dot = (ci[:, 0] * c0[:, 0] + ci[:, 1] * c0[:, 1]) + ci[:, 2] * c0[:, 2]
                    keep = valid & (d0 != 0.0) & (leni > 0.0) & (len0 > 0.0) & (dot >= cos_max * (leni * len0))
                    w = d0 / cand_d[:, i]
                sel = np.nonzero(keep)[0]
                idx[b + sel, pos[sel]] = cand_g[sel, i]
                d2o[b + sel, pos[sel]] = cand_d[sel, i]
                wi[sel, pos[sel]] = w[sel]
                W[sel] = W[sel] + w[sel]
                pos[sel] += 1
            live = pos > 0
            wo[b:b + B][live] = wi[live] / W[live, None]
            count[b:b + B] = pos
    return idx, d2o, wo, count


def blend_numpy(gp, ga, roots, idx, w, kept):
    """(points [n_kept M, 3], attrs [n_kept M, C]) float32 of the roots `kept`."""
    K, M, C = gp.shape[0], gp.shape[1], ga.shape[2]
    k, n_kept = idx.shape[1], kept.shape[0]
    pts, att = np.empty((n_kept, M, 3), np.float32), np.empty((n_kept, M, C), np.float32)
    step = max(1, _BUDGET // (M * max(3, C)))
    with np.errstate(all="ignore"):
        for b in range(0, n_kept, step):
            rows = kept[b:b + step]
            accp, acca = np.zeros((rows.shape[0], M, 3), np.float64), np.zeros((rows.shape[0], M, C), np.float64)
            for i in range(k):
                g = idx[rows, i]
                sel = np.nonzero(g >= 0)[0]
                if sel.size == 0:
                    break                              # (compacted rows: no later slot is filled either)
                p = gp[g[sel]].astype(np.float64)
                wt = w[rows[sel], i][:, None, None]
                accp[sel] = accp[sel] + wt * (p - p[:, :1])
                acca[sel] = acca[sel] + wt * ga[g[sel]].astype(np.float64)
            pts[b:b + step] = (roots[rows][:, None, :] + accp).astype(np.float32)
            att[b:b + step] = acca.astype(np.float32)
    return pts.reshape(n_kept * M, 3), att.reshape(n_kept * M, C)


# ---- device path -----------------------------------------------------------------------------------------------------------------
def search_device(gp, roots, k, max_d2, cos_max):
    """hgs_groom_neighbours on device tensors (gp float32 [K, M, 3], roots float64 [N, 3]): (idx, d2, w, count) on the device."""
    import hgs_runtime as rt
    gp = rt.require_gpu_tensor(gp, "guide points", torch.float32)
    roots = rt.require_gpu_tensor(roots, "roots", torch.float64)
    if gp.dim() != 3 or gp.shape[2] != 3 or roots.dim() != 2 or roots.shape[1] != 3:
        raise rt.HgsError(f"search_device: guide points {tuple(gp.shape)} and roots {tuple(roots.shape)}; [K, M, 3] and [N, 3] expected")
    N, K, M, k = int(roots.shape[0]), int(gp.shape[0]), int(gp.shape[1]), int(k)
    dev = roots.device
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((N, k), dtype=torch.float64, device=dev)
    w = torch.empty((N, k), dtype=torch.float64, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_groom_neighbours(rt.current_stream(), N, rt.ptr(roots), K, M, rt.ptr(gp), k, float(max_d2), float(cos_max),
                                               rt.ptr(idx), rt.ptr(d2), rt.ptr(w), rt.ptr(count)))
    return idx, d2, w, count


def blend_device(gp, ga, roots, idx, w, kept):
    """hgs_groom_blend: (points [n_kept M, 3], attrs [n_kept M, C]) float32 on the device; kept: int32 [n_kept], ascending root numbers
    (interpolate_strands builds it from `count`; the kernel is not told N and trusts it)."""
    import hgs_runtime as rt
    gp = rt.require_gpu_tensor(gp, "guide points", torch.float32)
    ga = rt.require_gpu_tensor(ga, "guide attributes", torch.float32)
    roots = rt.require_gpu_tensor(roots, "roots", torch.float64)
    idx = rt.require_device_buffer(idx, "idx", torch.int32)
    w = rt.require_device_buffer(w, "w", torch.float64)
    kept = rt.require_device_buffer(kept, "kept", torch.int32)
    if gp.dim() != 3 or gp.shape[2] != 3 or ga.dim() != 3 or roots.dim() != 2 or roots.shape[1] != 3 or idx.dim() != 2 or kept.dim() != 1:
        raise rt.HgsError(f"blend_device: guide points {tuple(gp.shape)}, attributes {tuple(ga.shape)}, roots {tuple(roots.shape)}, idx {tuple(idx.shape)}, "
                          f"kept {tuple(kept.shape)}; [K, M, 3], [K, M, C], [N, 3], [N, k] and [n_kept] expected")
    N, K, M, C, k, n_kept = int(roots.shape[0]), int(gp.shape[0]), int(gp.shape[1]), int(ga.shape[2]), int(idx.shape[1]), int(kept.numel())
    if tuple(ga.shape[:2]) != (K, M) or tuple(idx.shape) != (N, k) or tuple(w.shape) != (N, k):
        raise rt.HgsError(f"blend_device: attributes {tuple(ga.shape)}, idx {tuple(idx.shape)}, w {tuple(w.shape)} for {K} guides of {M} points and {N} roots")
    if n_kept and (int(kept.min()) < 0 or int(kept.max()) >= N):
        raise rt.HgsError(f"blend_device: a kept root is out of range of the {N} roots")
    dev = roots.device
    pts = torch.empty((n_kept * M, 3), dtype=torch.float32, device=dev)
    att = torch.empty((n_kept * M, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_groom_blend(rt.current_stream(), K, M, C, rt.ptr(gp), rt.ptr(ga), rt.ptr(roots), k, rt.ptr(idx), rt.ptr(w),
                                          n_kept, rt.ptr(kept), rt.ptr(pts), rt.ptr(att)))
    return pts, att


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def guide_arrays(guides):
    """(gp [K, M, 3], ga [K, M, C]) views of a StrandExport whose strands all have M points; ragged strands (native mode) are refused."""
    off = np.asarray(guides.offsets, np.int64)
    K = off.shape[0] - 1
    n = off[1:] - off[:-1]
    if K and np.any(n != n[0]):
        raise ValueError("interpolate_strands: the guides have different numbers of points (native mode, points = 0); resample them to a "
                         "fixed number of points")
    C = guides.attrs.shape[1]
    M = int(n[0]) if K else 2
    return (np.ascontiguousarray(guides.points, np.float32).reshape(K, M, 3), np.ascontiguousarray(guides.attrs, np.float32).reshape(K, M, C))


def polyline_length(pts):
    """float64 [n] lengths of float32 polylines [n, M, 3], added up in segment order."""
    d = pts[:, 1:].astype(np.float64) - pts[:, :-1].astype(np.float64)
    return np.cumsum(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]), axis=1)[:, -1]


def interpolate_strands(guides, roots, k=4, max_guide_distance=None, max_angle=60.0, device=None, first_id=None):
    """A strand for every root of `roots` (float64 [N, 3]) blended from the `k` nearest strands of `guides` (a StrandExport of a
    fixed number of points per strand), see the module docstring.  Returns a Groom of host arrays.  device=None: numpy; "cuda":
    the HIP kernels.  first_id: number of the first root's strand (default: one past the largest guide id)."""
    gp, ga = guide_arrays(guides)
    roots = np.ascontiguousarray(roots, np.float64)
    _check(gp, ga, roots, k)
    k = int(k)
    max_d2, cos_max = search_parameters(max_guide_distance, max_angle)
    N, M, C = roots.shape[0], gp.shape[1], ga.shape[2]
    if first_id is None:
        first_id = int(np.max(guides.strand_ids)) + 1 if len(guides.strand_ids) else 0
    if device is None:
        idx, _, w, count = search_numpy(gp, roots, k, max_d2, cos_max)
        kept = np.nonzero(count > 0)[0].astype(np.int64)
        pts, att = blend_numpy(gp, ga, roots, idx, w, kept)
    else:
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernels)")
        gp_d, ga_d, roots_d = (torch.as_tensor(a, device=device) for a in (gp, ga, roots))     # uploaded once
        idx_d, _, w_d, count_d = search_device(gp_d, roots_d, k, max_d2, cos_max)
        kept_d = torch.nonzero(count_d > 0).reshape(-1).to(torch.int32)
        pts_d, att_d = blend_device(gp_d, ga_d, roots_d, idx_d, w_d, kept_d)
        kept, count = kept_d.cpu().numpy().astype(np.int64), count_d.cpu().numpy()
        pts, att = pts_d.cpu().numpy(), att_d.cpu().numpy()
    n_kept = kept.shape[0]
    with np.errstate(all="ignore"):
        length = polyline_length(pts.reshape(n_kept, M, 3))
    strands = StrandExport(pts, att, np.arange(n_kept + 1, dtype=np.int64) * M, int(first_id) + kept, length)
    return Groom(strands, kept, int(N - n_kept), count[kept].astype(np.int32))


def concatenate(a, b):
    """The strands of two StrandExports in one, a's first."""
    return StrandExport(np.concatenate([a.points, b.points]), np.concatenate([a.attrs, b.attrs]),
                        np.concatenate([a.offsets, a.offsets[-1] + b.offsets[1:]]).astype(np.int64),
                        np.concatenate([a.strand_ids, b.strand_ids]).astype(np.int64), np.concatenate([a.length, b.length]))
