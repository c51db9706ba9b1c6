"""Exported strands rooted on the head (export_strands.py --attach_roots): Stage II assembles strands wherever a view saw hair and
Stage III grows their tips, but nothing connects a strand's root end to the head, so an exported strand begins millimetres to
centimetres above the skin.  From every strand's root joint a polyline is marched back to the head's surface: it starts along the
strand's own backward tangent, is steered by the direction volume of trace_strands.py --field (utils/trace.py, with utils/field_fill.py's
fill between the scalp and the visible hair) where one is given and has data, and is always pulled down the gradient of the head's
distance field (utils/head_sdf.py), so that it must arrive.  The new joints are put in front of the strand's own.

The contract (this module's numpy path, csrc/hgs_attach.hip and the loop restatement in tests/attach_reference.py state the same
thing).  It follows scene/strand_collide.py's conventions: all strand arithmetic is float64 with one rounding per operation, in exactly
the order written; dot(u, v) = (u0*v0 + u1*v1) + u2*v2; the head's field is sampled as S(x) of the collide contract (float32, at
float32(x): (ok, d, G), G the gradient converted to float64); the direction volume is sampled by the corner loop of utils/trace.py's
Trace statement (t = (x - origin)*k with k = 1/h divided once, w, v, the signs chosen against p); the kernel file is built with
-ffp-contract=off.

Inputs.  points float32 [P, 3], offsets int64 [K + 1] (as for the push-out).  A HeadSDF, at least 2 nodes an axis.  Optionally a
utils.trace.Field.  margin float32, finite, >= 0: the target distance above the head.  tol float32, finite, >= 0; the default is
float32(1e-3 * spacing).  step float64, finite, > 0; the default is 0.5 * spacing.  max_steps 1..1024 (256).  land_iters 1..8 (4).
pull finite, >= 0 (1).  descent in (0, 1] (0.25): the least cosine between a step and the way down.  max_distance >= 0 or None (+inf).
min_conf finite (0.5).  Below, m = (double)margin and tl = (double)tol.

Per strand with joints p_0 .. p_{n-1}:
    n < 2: DEGENERATE.  x = (double)p_0;  (ok, d, G) = S(x).
    not ok: RANGE.   (double)d <= m + tl: NEAR (already rooted).   (double)d - m > max_distance: FAR.
    e = x - (double)p_1;  le = sqrt(dot(e, e));  p = e/le if le is finite and > 0, else p = -G/gn with gn = sqrt(dot(G, G))
    repeat at most max_steps times:
        gn = sqrt(dot(G, G));  unless finite and > 0: FLAT
        if (double)d - m <= step:                                              # the landing
            repeat at most land_iters times:
                c = (m - (double)d)/gn;  x_k = x_k + (c*G_k)/gn per coordinate;  (ok, d, G) = S(x);  not ok: RANGE
                if |(double)d - m| <= tl: append x; REACHED
                gn = sqrt(dot(G, G));  unless finite and > 0: FLAT
            UNLANDED
        nrm = -G/gn
        f = the volume's direction v/sqrt(nn) at x, if a volume is given, x is in its range (every t finite and 0 <= t < n_axis - 1),
            w >= min_conf and nn = dot(v, v) is finite and > 0; otherwise f = p
        v = f + pull*nrm;  dd = v/sqrt(dot(v, v)) if that length is finite and > 0, else nrm
        if dot(dd, nrm) < descent: dd = nrm
        x = x + step*dd;  p = dd;  append x;  (ok, d, G) = S(x);  not ok: RANGE
    STEPS
Reason codes: REACHED 0, NEAR 1, DEGENERATE 2, RANGE 3, FLAT 4, STEPS 5, UNLANDED 6, FAR 7.  OFF_SCALP 8 is set on the host
(attach_roots: a landed root farther than scalp_distance from every scalp point).  The march's outputs: ext float64 [K, max_steps + 1,
3] (the appended points in order; rows from count on are unspecified), count int32 [K] (points appended, whatever the reason), reason
int32 [K], landed float32 [K]: d at the landed point (REACHED) or at the root (NEAR), +inf otherwise.  The range tests come before
every load, and negating any entries of the volume's dir changes no bit (a*e_j = (-a)*(-e_j); dot(e, p) == 0 exactly aside).

Rejoin.  Only REACHED changes a strand: its output is the appended joints in reverse order (the landed point first), each rounded once
to float32, followed by the original joints with their original bits; the new joints carry the root joint's attributes.  With M >= 2 a
REACHED strand is resampled to M points by scene/strand_export.py's statement applied to that plain polyline v_0 .. v_{m-1}: len_i =
sqrt(dot(v_{i+1} - v_i, ..)) in float64 of the float32 joints, cum_0 = 0 and cum_{i+1} = cum_i + len_i in segment order, L = cum_{m-1};
sample 0 and sample M - 1 are the end joints' bits; inner sample j has t = (j/(M-1)) L, i = the largest index <= m - 2 with cum_i <= t
(0 where there is none), w = (t - cum_i)/len_i if len_i > 0 else 0, v_i + w (v_{i+1} - v_i) and a_i + w (a_{i+1} - a_i) with the joints'
own attributes (no segment averaging), rounded once to float32.  Every other strand is copied, whatever its size.  `length` is
recomputed by strand_collide.strand_lengths.

Known limits.  Euler stepping.  Only the root joint's attributes are extended.  The landing is on the *head*: the scalp test is a
distance to the scalp points, not a region of the mesh.  Models are not re-rooted for training: the step works on exported strands
only.

device=None: numpy, vectorised over the strands still marching, with explicit loops over the steps and the landing iterations.
device="cuda": hgs_root_attach and hgs_strand_rejoin on torch tensors.  The caller chooses; neither falls back to the other."""
import math
from typing import NamedTuple

import numpy as np

from scene.strand_collide import _check_points, check_offsets, strand_lengths
from scene.strand_export import StrandExport
from utils import head_sdf
from utils.trace import BUDGET, batch_roots

REACHED, NEAR, DEGENERATE, RANGE, FLAT, STEPS, UNLANDED, FAR, OFF_SCALP = range(9)
REASONS = ("reached", "near", "degenerate", "range", "flat", "steps", "unlanded", "far", "off_scalp")
MAX_STEPS, MAX_LAND, MAX_CHANNELS = 1024, 8, 64
_BLOCK = 1 << 21          # elements of one vectorised block of the rejoin (strands x padded joints)


class Knobs(NamedTuple):
    margin: np.float32
    tol: np.float32
    step: float
    max_steps: int
    land_iters: int
    pull: float
    descent: float
    max_distance: float
    min_conf: float


def default_tol(sdf):
    return np.float32(1e-3 * sdf.spacing)


def check_parameters(sdf, margin=0.0, tol=None, step=None, max_steps=256, land_iters=4, pull=1.0, descent=0.25, max_distance=None,
                     min_conf=0.5):
    """The Knobs of the contract, or ValueError."""
    if min(sdf.shape) < 2:
        raise ValueError(f"a field of {sdf.shape} nodes: at least 2 an axis")
    margin = np.float32(margin)
    tol = default_tol(sdf) if tol is None else np.float32(tol)
    step = 0.5 * sdf.spacing if step is None else float(step)
    pull, descent, min_conf = float(pull), float(descent), float(min_conf)
    max_distance = math.inf if max_distance is None else float(max_distance)
    if not (np.isfinite(margin) and margin >= 0):
        raise ValueError(f"margin = {margin}: finite and >= 0")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol = {tol}: finite and >= 0")
    if not (math.isfinite(step) and step > 0.0):
        raise ValueError(f"step = {step}: finite and > 0")
    if int(max_steps) != max_steps or not 1 <= int(max_steps) <= MAX_STEPS:
        raise ValueError(f"max_steps = {max_steps}: 1 to {MAX_STEPS}")
    if int(land_iters) != land_iters or not 1 <= int(land_iters) <= MAX_LAND:
        raise ValueError(f"land_iters = {land_iters}: 1 to {MAX_LAND}")
    if not (math.isfinite(pull) and pull >= 0.0):
        raise ValueError(f"pull = {pull}: finite and >= 0")
    if not 0.0 < descent <= 1.0:
        raise ValueError(f"descent = {descent}: above 0, at most 1")
    if not max_distance >= 0.0:
        raise ValueError(f"max_distance = {max_distance}: >= 0, or None")
    if not math.isfinite(min_conf):
        raise ValueError(f"min_conf = {min_conf}: finite")
    return Knobs(margin, tol, step, int(max_steps), int(land_iters), pull, descent, max_distance, min_conf)


def _check_attrs(attrs, P):
    attrs = np.asarray(attrs)
    if attrs.ndim != 2 or attrs.shape[0] != P or attrs.shape[1] > MAX_CHANNELS:
        raise ValueError(f"attrs of shape {attrs.shape}: [{P}, C] with at most {MAX_CHANNELS} channels expected")
    return np.ascontiguousarray(attrs, dtype=np.float32)


# ---- numpy path: the march ---------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sample(x, sdf):
    """S(x) for float64 coordinate columns: (ok, d float32, d as float64, [G0, G1, G2] float64)."""
    ok, d, gx, gy, gz = head_sdf.trilinear(np.stack(x, axis=1).astype(np.float32), sdf)
    return ok, d, d.astype(np.float64), [g.astype(np.float64) for g in (gx, gy, gz)]


def _positive(v):
    return np.isfinite(v) & (v > 0.0)


def _steer(field, x, p, min_conf):
    """(on, [f0, f1, f2]): the volume's direction at the columns x, sign-aligned to p -- utils/trace.py's corner loop."""
    nx, ny, nz = field.shape
    o, k = field.origin, 1.0 / field.spacing
    dirf, conff = field.dir.reshape(-1, 3), field.conf.reshape(-1)
    t = [(x[c] - o[c]) * k for c in range(3)]
    ok = np.ones(x[0].shape[0], bool)
    for c, n in enumerate((nx, ny, nz)):
        ok &= (t[c] >= 0.0) & (t[c] < np.float64(n - 1))                      # (a NaN fails every comparison, +inf the second)
    t = [np.where(ok, v, 0.0) for v in t]                                     # (rows out of range: any valid address)
    fl = [np.floor(v) for v in t]
    i = [v.astype(np.int64) for v in fl]
    f = [t[c] - fl[c] for c in range(3)]
    g = [1.0 - f[c] for c in range(3)]
    base = (i[2] * ny + i[1]) * nx + i[0]
    w = np.zeros(base.shape[0], np.float64)
    v = [np.zeros(base.shape[0], np.float64) for _ in range(3)]
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                at = base + (cz * ny + cy) * nx + cx
                tw = ((f[0] if cx else g[0]) * (f[1] if cy else g[1])) * (f[2] if cz else g[2])
                a = tw * conff[at]
                w = w + a
                e = dirf[at]
                a = np.where(_dot(e.T, p) < 0.0, -a, a)
                v = [v[j] + a * e[:, j] for j in range(3)]
    nn = _dot(v, v)
    on = ok & (w >= min_conf) & _positive(nn)
    ln = np.sqrt(nn)
    return on, [v[j] / ln for j in range(3)]


def attach_numpy(points, offsets, sdf, field=None, **knobs):
    """(ext float64 [K, max_steps + 1, 3], count int32 [K], reason int32 [K], landed float32 [K]) of the contract's march; rows of ext
    from count on are zero."""
    points = _check_points(points)
    off = check_offsets(offsets, points.shape[0])
    q = check_parameters(sdf, **knobs)
    K = off.shape[0] - 1
    ext = np.zeros((K, q.max_steps + 1, 3), np.float64)
    count = np.zeros(K, np.int32)
    reason = np.full(K, DEGENERATE, np.int32)
    landed = np.full(K, np.inf, np.float32)
    n = off[1:] - off[:-1]
    S = np.nonzero(n >= 2)[0]                                                   # the strands still marching, ascending
    if S.size == 0:
        return ext, count, reason, landed
    m, tl = np.float64(q.margin), np.float64(q.tol)

    def keep(mask, *cols):
        return tuple([v[mask] for v in c] if isinstance(c, list) else c[mask] for c in cols)

    def append(rows, x):
        for c in range(3):
            ext[rows, count[rows], c] = x[c]
        count[rows] += 1

    with np.errstate(all="ignore"):
        x = [points[off[S], c].astype(np.float64) for c in range(3)]
        ok, d32, d, G = _sample(x, sdf)
        near = ok & (d <= m + tl)
        far = ok & ~near & (d - m > q.max_distance)
        reason[S[~ok]], reason[S[near]], reason[S[far]] = RANGE, NEAR, FAR
        landed[S[near]] = d32[near]
        S, x, d, G = keep(ok & ~near & ~far, S, x, d, G)
        e = [x[c] - points[off[S] + 1, c].astype(np.float64) for c in range(3)]
        le, g0 = np.sqrt(_dot(e, e)), np.sqrt(_dot(G, G))
        own = _positive(le)
        p = [np.where(own, e[c] / le, -G[c] / g0) for c in range(3)]
        reason[S] = STEPS
        for _ in range(q.max_steps):
            if S.size == 0:
                break
            gn = np.sqrt(_dot(G, G))
            flat = ~_positive(gn)
            reason[S[flat]] = FLAT
            land = ~flat & (d - m <= q.step)
            if land.any():                                                      # the landing, to its end
                A, xa, da, Ga, ga = keep(land, S, x, d, G, gn)
                reason[A] = UNLANDED
                for _ in range(q.land_iters):
                    if A.size == 0:
                        break
                    c_ = (m - da) / ga
                    xa = [xa[c] + (c_ * Ga[c]) / ga for c in range(3)]
                    ok, d32, da, Ga = _sample(xa, sdf)
                    reason[A[~ok]] = RANGE
                    A, xa, d32, da, Ga = keep(ok, A, xa, d32, da, Ga)
                    hit = np.abs(da - m) <= tl
                    rows = A[hit]
                    append(rows, [v[hit] for v in xa])
                    reason[rows], landed[rows] = REACHED, d32[hit]
                    A, xa, da, Ga = keep(~hit, A, xa, da, Ga)
                    ga = np.sqrt(_dot(Ga, Ga))
                    bad = ~_positive(ga)
                    reason[A[bad]] = FLAT
                    A, xa, da, Ga, ga = keep(~bad, A, xa, da, Ga, ga)
            S, x, G, p, gn = keep(~flat & ~land, S, x, G, p, gn)
            if S.size == 0:
                break
            nrm = [-G[c] / gn for c in range(3)]
            f = p
            if field is not None:
                on, fv = _steer(field, x, p, q.min_conf)
                f = [np.where(on, fv[c], p[c]) for c in range(3)]
            v = [f[c] + q.pull * nrm[c] for c in range(3)]
            vn = np.sqrt(_dot(v, v))
            good = _positive(vn)
            dd = [np.where(good, v[c] / vn, nrm[c]) for c in range(3)]
            low = _dot(dd, nrm) < q.descent
            dd = [np.where(low, nrm[c], dd[c]) for c in range(3)]
            x = [x[c] + q.step * dd[c] for c in range(3)]
            p = dd
            append(S, x)
            ok, _, d, G = _sample(x, sdf)
            reason[S[~ok]] = RANGE
            S, x, d, G, p = keep(ok, S, x, d, G, p)
    return ext, count, reason, landed


# ---- numpy path: the rejoin --------------------------------------------------------------------------------------------------------
def _ranges(starts, sizes):
    """The concatenation of arange(starts[k], starts[k] + sizes[k])."""
    sizes = np.asarray(sizes, np.int64)
    total = int(sizes.sum())
    first = np.cumsum(sizes) - sizes
    return np.repeat(np.asarray(starts, np.int64) - first, sizes) + np.arange(total, dtype=np.int64)


def reached_mask(count, reason, n):
    return (np.asarray(reason) == REACHED) & (np.asarray(count) >= 1) & (n >= 1)


def out_sizes(offsets, count, reason, M):
    """(reached bool [K], out_offsets int64 [K + 1]) of the rejoin: n points for a strand that is copied, count + n (M == 0) or M for
    a REACHED one."""
    off = np.asarray(offsets, np.int64)
    n = off[1:] - off[:-1]
    reached = reached_mask(count, reason, n)
    size = np.where(reached, np.int64(M) if M else n + np.asarray(count, np.int64), n)
    return reached, np.concatenate([[0], np.cumsum(size)]).astype(np.int64)


def _check_rejoin(points, attrs, offsets, ext, count, reason, M):
    points = _check_points(points)
    attrs = _check_attrs(attrs, points.shape[0])
    off = check_offsets(offsets, points.shape[0])
    K = off.shape[0] - 1
    M = int(M)
    if M < 0 or M == 1:
        raise ValueError(f"M = {M}: 0 for the joints themselves, else at least 2 points per strand")
    ext, count, reason = np.asarray(ext), np.asarray(count), np.asarray(reason)
    if ext.ndim != 3 or ext.shape[0] != K or ext.shape[2] != 3 or not 2 <= ext.shape[1] <= MAX_STEPS + 1 or ext.dtype != np.float64:
        raise ValueError(f"ext of shape {ext.shape} and type {ext.dtype}: float64 [{K}, max_steps + 1, 3] expected")
    if count.shape != (K,) or reason.shape != (K,) or count.dtype != np.int32 or reason.dtype != np.int32:
        raise ValueError(f"count {count.shape} {count.dtype} and reason {reason.shape} {reason.dtype}: int32 [{K}] expected")
    if K and (count.min() < 0 or count.max() > ext.shape[1]):
        raise ValueError(f"count outside 0 .. {ext.shape[1]}")
    return points, attrs, off, ext, count, reason, M


def rejoin_numpy(points, attrs, offsets, ext, count, reason, M=0):
    """(out_points float32 [N, 3], out_attrs float32 [N, C], out_offsets int64 [K + 1]) of the contract's rejoin."""
    points, attrs, off, ext, count, reason, M = _check_rejoin(points, attrs, offsets, ext, count, reason, M)
    C = attrs.shape[1]
    n = off[1:] - off[:-1]
    reached, out_off = out_sizes(off, count, reason, M)
    out = np.empty((int(out_off[-1]), 3), np.float32)
    oat = np.empty((int(out_off[-1]), C), np.float32)
    T = np.nonzero(~reached)[0]                                                 # copied
    src, dst = _ranges(off[T], n[T]), _ranges(out_off[T], n[T])
    out[dst], oat[dst] = points[src], attrs[src]
    R = np.nonzero(reached)[0]
    cnt = count.astype(np.int64)
    if M == 0:
        k = np.repeat(R, cnt[R])
        j = _ranges(np.zeros(R.shape[0], np.int64), cnt[R])
        with np.errstate(all="ignore"):
            out[out_off[k] + j] = ext[k, cnt[k] - 1 - j].astype(np.float32)
        oat[out_off[k] + j] = attrs[off[k]]
        src, dst = _ranges(off[R], n[R]), _ranges(out_off[R] + cnt[R], n[R])
        out[dst], oat[dst] = points[src], attrs[src]
        return out, oat, out_off
    attr64 = attrs.astype(np.float64)
    frac = np.arange(M, dtype=np.float64) / np.float64(M - 1)
    pos = 0
    with np.errstate(all="ignore"):
        while pos < R.shape[0]:
            widest = int((n[R[pos:]] + cnt[R[pos:]]).max())
            rows = R[pos:pos + max(1, _BLOCK // (max(widest, M) * max(3, C)))]
            pos += rows.shape[0]
            c_, n_, o_ = cnt[rows][:, None], n[rows][:, None], off[rows][:, None]
            mm = c_ + n_                                                       # joints of the joined polyline, >= 2
            width = int(mm.max())
            i = np.arange(width, dtype=np.int64)[None, :]
            new = i < c_
            J = np.where(new[..., None], ext[rows[:, None], np.clip(c_ - 1 - i, 0, None)].astype(np.float32),
                         points[o_ + np.clip(i - c_, 0, n_ - 1)]).astype(np.float64)
            e = J[:, 1:] - J[:, :-1]
            seg = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
            cum = np.concatenate([np.zeros((rows.shape[0], 1)), np.cumsum(np.where(i[:, 1:] < mm, seg, 0.0), axis=1)], axis=1)
            r = np.arange(rows.shape[0])[:, None]
            t = frac[None, :] * cum[r, mm - 1]
            lo, hi = np.zeros(t.shape, np.int64), np.broadcast_to(mm - 1, t.shape).copy()
            while True:                                                         # the largest i <= m - 2 with cum_i <= t, 0 if none
                act = hi - lo > 1
                if not act.any():
                    break
                mid = (lo + hi) >> 1
                le = cum[r, mid] <= t
                lo, hi = np.where(act & le, mid, lo), np.where(act & ~le, mid, hi)
            va, vb, sl = J[r, lo], J[r, lo + 1], seg[r, lo]
            w = np.divide(t - cum[r, lo], sl, out=np.zeros_like(t), where=sl > 0)
            p = (va + w[..., None] * (vb - va)).astype(np.float32)
            a0, a1 = attr64[o_ + np.maximum(lo - c_, 0)], attr64[o_ + np.maximum(lo + 1 - c_, 0)]
            a = (a0 + w[..., None] * (a1 - a0)).astype(np.float32)
            p[:, 0], p[:, M - 1] = J[:, 0].astype(np.float32), points[off[rows] + n[rows] - 1]
            a[:, 0], a[:, M - 1] = attrs[off[rows]], attrs[off[rows] + n[rows] - 1]
            dst = out_off[rows][:, None] + np.arange(M)[None, :]
            out[dst], oat[dst] = p, a
    return out, oat, out_off


# ---- device path -------------------------------------------------------------------------------------------------------------------
def volume_on(field, device):
    """The direction volume's device copy for attach_device: (dir, conf, origin, spacing, shape), or None."""
    if field is None:
        return None
    import torch
    return torch.from_numpy(field.dir).to(device), torch.from_numpy(field.conf).to(device), field.origin, field.spacing, field.shape


def attach_device(points, offsets, sdf, volume=None, **knobs):
    """hgs_root_attach on device tensors (points float32 [P, 3], offsets int64 [K + 1], already checked: check_offsets; volume: what
    volume_on returns): (ext, count, reason, landed) on the device."""
    import torch
    import hgs_runtime as rt
    points = rt.require_gpu_tensor(points, "points", torch.float32)
    offsets = rt.require_gpu_tensor(offsets, "offsets", torch.int64)
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise rt.HgsError(f"attach_device: points {tuple(points.shape)} and offsets {tuple(offsets.shape)}; [P, 3] and [K + 1] expected")
    try:
        q = check_parameters(sdf, **knobs)
    except ValueError as e:
        raise rt.HgsError(f"attach_device: {e}") from None
    P, K, dev = int(points.shape[0]), int(offsets.shape[0]) - 1, points.device
    head = sdf.on(dev)
    nx, ny, nz = sdf.shape
    if head["phi"].numel() != nx * ny * nz:
        raise rt.HgsError(f"attach_device: a field of {head['phi'].numel()} values for a grid of {nx} x {ny} x {nz} nodes")
    if volume is None:
        vol = (None, None, 2, 2, 2, 0.0, 0.0, 0.0, 1.0)
    else:
        vdir, vconf, vo, vh, vshape = volume
        rt.trace_check(shape=vshape, dir=vdir, conf=vconf)
        if vdir.device != dev or vconf.device != dev:
            raise rt.HgsError("attach_device: the volume lives on another device than the points")
        vol = (rt.ptr(vdir), rt.ptr(vconf), int(vshape[0]), int(vshape[1]), int(vshape[2]), float(vo[0]), float(vo[1]), float(vo[2]), float(vh))
    ext = torch.empty((K, q.max_steps + 1, 3), dtype=torch.float64, device=dev)
    count = torch.zeros(K, dtype=torch.int32, device=dev)
    reason = torch.zeros(K, dtype=torch.int32, device=dev)
    landed = torch.zeros(K, dtype=torch.float32, device=dev)
    o = sdf.origin32
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_root_attach(rt.current_stream(), K, rt.ptr(offsets), P, rt.ptr(points), rt.ptr(head["phi"]), nx, ny, nz,
                                          float(o[0]), float(o[1]), float(o[2]), float(sdf.inv_h32), *vol, q.min_conf, float(q.margin),
                                          float(q.tol), q.step, q.max_steps, q.land_iters, q.pull, q.descent, q.max_distance, rt.ptr(ext),
                                          rt.ptr(count), rt.ptr(reason), rt.ptr(landed)))
    return ext, count, reason, landed


def rejoin_device(points, attrs, offsets, ext, count, reason, M, out_offsets, n_out):
    """hgs_strand_rejoin on device tensors: (out_points float32 [n_out, 3], out_attrs float32 [n_out, C]).  out_offsets is the [K + 1]
    int64 device tensor of out_sizes, n_out its last entry, which the caller passes (reading it here would be a synchronisation)."""
    import torch
    import hgs_runtime as rt
    points = rt.require_gpu_tensor(points, "points", torch.float32)
    attrs = rt.require_gpu_tensor(attrs, "attrs", torch.float32)
    offsets = rt.require_gpu_tensor(offsets, "offsets", torch.int64)
    out_offsets = rt.require_gpu_tensor(out_offsets, "out_offsets", torch.int64)
    ext = rt.require_device_buffer(ext, "ext", torch.float64)
    count = rt.require_device_buffer(count, "count", torch.int32)
    reason = rt.require_device_buffer(reason, "reason", torch.int32)
    P, K, M, n_out = int(points.shape[0]), int(offsets.shape[0]) - 1, int(M), int(n_out)
    if points.dim() != 2 or points.shape[1] != 3 or attrs.dim() != 2 or attrs.shape[0] != P or attrs.shape[1] > MAX_CHANNELS:
        raise rt.HgsError(f"rejoin_device: points {tuple(points.shape)} and attrs {tuple(attrs.shape)}; [P, 3] and [P, C <= {MAX_CHANNELS}] expected")
    if K < 0 or out_offsets.shape != (K + 1,) or count.shape != (K,) or reason.shape != (K,) or ext.dim() != 3 or ext.shape[0] != K \
            or ext.shape[2] != 3 or not 2 <= ext.shape[1] <= MAX_STEPS + 1:
        raise rt.HgsError(f"rejoin_device: {K} strands with out_offsets {tuple(out_offsets.shape)}, count {tuple(count.shape)}, reason "
                          f"{tuple(reason.shape)} and ext {tuple(ext.shape)}")
    if M < 0 or M == 1 or n_out < 0:
        raise rt.HgsError(f"rejoin_device: M = {M} (0, or at least 2) and n_out = {n_out} (>= 0)")
    C, dev = int(attrs.shape[1]), points.device
    out = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    oat = torch.empty((n_out, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_strand_rejoin(rt.current_stream(), K, rt.ptr(offsets), P, rt.ptr(points), rt.ptr(attrs), C, rt.ptr(ext),
                                            int(ext.shape[1]), rt.ptr(count), rt.ptr(reason), M, rt.ptr(out_offsets), n_out, rt.ptr(out),
                                            rt.ptr(oat)))
    return out, oat


# ---- entry point -------------------------------------------------------------------------------------------------------------------
def _off_scalp(roots, scalp_points, scalp_distance):
    """bool [R]: the float32 landed roots farther than scalp_distance from every scalp point.  Host arithmetic on both paths."""
    import torch
    from scene.hair_gaussian_model import nearest_distance
    if roots.shape[0] == 0:
        return np.zeros(0, bool)
    dist = nearest_distance(torch.from_numpy(np.ascontiguousarray(roots, np.float32)),
                            torch.from_numpy(np.ascontiguousarray(scalp_points, np.float64))).numpy()
    return ~(dist <= float(scalp_distance))


def select_strands(strands, keep):
    """The StrandExport of the strands `keep` (bool [K]) names, in order."""
    off = np.asarray(strands.offsets, np.int64)
    kept = np.nonzero(keep)[0]
    n = (off[1:] - off[:-1])[kept]
    rows = _ranges(off[kept], n)
    return StrandExport(strands.points[rows], strands.attrs[rows], np.concatenate([[0], np.cumsum(n)]).astype(np.int64),
                        np.asarray(strands.strand_ids)[kept], np.asarray(strands.length)[kept])


def attach_roots(strands, sdf, field=None, points=0, scalp_points=None, scalp_distance=None, device=None, budget=BUDGET, **knobs):
    """`strands` (a StrandExport, ragged or not) with every strand marched back to the head of `sdf` (a HeadSDF), steered by `field`
    (a utils.trace.Field or None), see the module docstring: (StrandExport, report).  points = M: 0 joins, M >= 2 resamples the
    joined strands to M points.  scalp_points [N, 3] with scalp_distance: a landed root farther than that from every scalp point is
    OFF_SCALP and its strand restored.  The strands are marched in batches whose `ext` fits `budget` bytes (utils/trace.py's rule).
    report: "strands", "attached", "near", "failed" (reason name -> strands, the failing reasons), "joints_added", "gap_max",
    "gap_mean" (the roots' distance above the margin before, over the roots in the field's range), "landed_error" (the largest
    |d - margin| of the landed roots) and "reason" (int32 [K])."""
    pts = _check_points(strands.points)
    att = _check_attrs(strands.attrs, pts.shape[0])
    off = check_offsets(strands.offsets, pts.shape[0])
    q = check_parameters(sdf, **knobs)
    M = int(points)
    if M < 0 or M == 1:
        raise ValueError(f"points = {points}: 0 for the joined joints, else at least 2 points per strand")
    if (scalp_distance is None) != (scalp_points is None):
        raise ValueError("scalp_points and scalp_distance come together, or neither")
    if scalp_distance is not None:
        scalp_points = np.asarray(scalp_points, np.float64).reshape(-1, 3)
        if not float(scalp_distance) >= 0.0 or scalp_points.shape[0] == 0:
            raise ValueError(f"scalp_distance = {scalp_distance} (>= 0) over {scalp_points.shape[0]} scalp points (at least one)")
    cuda = device is not None
    if cuda:
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernels)")
        import torch
        volume = volume_on(field, device)
    K = off.shape[0] - 1
    B = batch_roots(q.max_steps, budget)
    parts, reasons, landeds, added = [], [], [], 0
    for s0 in range(0, K, B):
        s1 = min(K, s0 + B)
        a, b = int(off[s0]), int(off[s1])
        p_, a_, o_ = pts[a:b], att[a:b], off[s0:s1 + 1] - a
        if cuda:
            p_d, a_d, o_d = (torch.as_tensor(v, device=device) for v in (p_, a_, o_))
            ext, count_d, reason_d, landed_d = attach_device(p_d, o_d, sdf, volume, **knobs)
            count, reason, landed = count_d.cpu().numpy(), reason_d.cpu().numpy(), landed_d.cpu().numpy()
        else:
            ext, count, reason, landed = attach_numpy(p_, o_, sdf, field, **knobs)
        if scalp_distance is not None:
            hit = np.nonzero(reason == REACHED)[0]
            if cuda:
                rows = torch.as_tensor(hit, device=device)
                last = ext[rows, (count_d[rows] - 1).to(torch.int64)].cpu().numpy()
            else:
                last = ext[hit, count[hit] - 1]
            with np.errstate(all="ignore"):
                reason[hit[_off_scalp(last.astype(np.float32), scalp_points, scalp_distance)]] = OFF_SCALP
        reached, out_off = out_sizes(o_, count, reason, M)
        if cuda:
            out_d, oat_d = rejoin_device(p_d, a_d, o_d, ext, count_d, torch.as_tensor(reason, device=device), M,
                                         torch.as_tensor(out_off, device=device), int(out_off[-1]))
            out, oat = out_d.cpu().numpy(), oat_d.cpu().numpy()
        else:
            out, oat, _ = rejoin_numpy(p_, a_, o_, ext, count, reason, M)
        parts.append((out, oat, out_off))
        reasons.append(reason)
        landeds.append(landed)
        added += int(count[reached].sum(dtype=np.int64))
    C = att.shape[1]
    out = np.concatenate([p[0] for p in parts] + [np.zeros((0, 3), np.float32)])
    oat = np.concatenate([p[1] for p in parts] + [np.zeros((0, C), np.float32)])
    base = np.cumsum([0] + [int(p[2][-1]) for p in parts])
    out_off = np.concatenate([np.zeros(1, np.int64)] + [p[2][1:] + base[k] for k, p in enumerate(parts)]).astype(np.int64)
    reason = np.concatenate(reasons + [np.zeros(0, np.int32)])
    landed = np.concatenate(landeds + [np.zeros(0, np.float32)])
    n = off[1:] - off[:-1]
    with np.errstate(all="ignore"):
        ok, d, _, _, _ = head_sdf.trilinear(pts[off[:-1][n >= 1]], sdf)
        gap = np.maximum(d[ok].astype(np.float64) - np.float64(q.margin), 0.0)
        gap = gap[np.isfinite(gap)]
        err = np.abs(landed[reason == REACHED].astype(np.float64) - np.float64(q.margin))
        length = strand_lengths(out, out_off)
    tally = np.bincount(reason, minlength=len(REASONS))
    report = dict(strands=K, attached=int(tally[REACHED]), near=int(tally[NEAR]),
                  failed={REASONS[r]: int(tally[r]) for r in range(2, len(REASONS)) if tally[r]}, joints_added=added,
                  gap_max=float(gap.max()) if gap.shape[0] else 0.0, gap_mean=float(gap.mean()) if gap.shape[0] else 0.0,
                  landed_error=float(err.max()) if err.shape[0] else 0.0, reason=reason)
    return StrandExport(out, oat, out_off, strands.strand_ids, length), report
