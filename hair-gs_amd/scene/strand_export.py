"""Strands of a trained model as runs of points, for the strand-file writers (data/strand_files.py, export_strands.py).

A trained strand has 1 to a few hundred unevenly long segments with per-segment attributes; every strand file format wants runs
of points, usually a fixed number per strand.  `resample_strands` resamples every strand of `model.strands_info` by arc length.

The contract (this path, csrc/hgs_export.hip and the tests' loop restatement state the same thing).  Inputs: the strands (offsets
[S+1], rows [total][2] endpoint ids root -> tip, the row of the segment table behind every strand row), the float32 endpoints and a
float32 per-segment attribute table attr[P][C] (`export_attributes`: RGB = clamp(0.5 + C0 f_dc, 0, 1), the activated opacity, the
width the model renders with, both rounded once from float64).  Strand s has n >= 1 segments and gets M >= 2 points; all arithmetic is float64 on the float32 inputs,
one rounding per operation:
    v_0..v_n            v_i = endpoints[rows[o+i][0]], v_n = endpoints[rows[o+n-1][1]]
    len_i               sqrt((dx*dx + dy*dy) + dz*dz)
    cum_0 = 0, cum_{i+1} = cum_i + len_i, L = cum_n                         (summed in segment order)
    a_0 = attr[seg_0], a_n = attr[seg_{n-1}], a_i = 0.5 (attr[seg_{i-1}] + attr[seg_i])
    sample 0 = (v_0, a_0), sample M-1 = (v_n, a_n), exactly
    inner sample j      t = (j / (M-1)) L;  i = the largest index with cum_i <= t, at most n-1;  w = (t - cum_i) / len_i, 0 if len_i = 0;
                        v_i + w (v_{i+1} - v_i),  a_i + w (a_{i+1} - a_i)
rounded once to float32.  A strand with L = 0 yields M copies of v_0.  points = 0 (native mode) does not resample: the output is the
joints themselves, n + 1 per strand, with the joint attributes.  Filters (min_segments, min_length, max_root_distance) are host
arithmetic on `length` and `offsets`; kept strands keep their order and the result names their original numbers.

device=None: numpy, vectorised over the strands (no Python loop per strand).  device="cuda": hgs_strand_arclen /
hgs_strand_resample on the model's device tensors and the strand tables the device walk left there.  The caller chooses; neither
falls back to the other (the convention of utils/normals.py and loss/metrics.py)."""
from typing import NamedTuple

import numpy as np
import torch

from utils.sh import C0

ATTRIBUTES = ("red", "green", "blue", "opacity", "width")


class StrandExport(NamedTuple):
    points: np.ndarray       # float32 [N, 3]
    attrs: np.ndarray        # float32 [N, C] (ATTRIBUTES for a model's export)
    offsets: np.ndarray      # int64 [K+1]: strand k owns points offsets[k]:offsets[k+1]
    strand_ids: np.ndarray   # int64 [K]: number of the kept strand in model.strands_info
    length: np.ndarray       # float64 [K]: arc length L

    @property
    def n_strands(self):
        return len(self.offsets) - 1


def export_attributes(model):
    """attr[P][5] of the whole segment table, float32, on the model's device (by torch, from the model's getters' definitions).
    The two activations -- the opacity's sigmoid, the width's exp -- are evaluated in float64 and rounded once: torch's float32
    sigmoid differs between the CPU and the GPU by up to two units in the last place, and the file a model exports should not
    depend on the device that wrote it (tests/test_strand_export_gpu.py compares the two drivers' files).  The values are within one
    float32 unit of get_opacity and get_scaling[:, 1], which the model renders with."""
    with torch.no_grad():
        P = int(model.endpoint_pairs.shape[0])
        rgb = torch.clamp(0.5 + C0 * model._features_dc.detach().reshape(P, 3), 0.0, 1.0)
        opacity = model.opacity_activation(model._opacity.detach().to(torch.float64)).to(torch.float32)
        width = model.scaling_activation(model._width.detach().to(torch.float64)).to(torch.float32)
        return torch.cat((rgb, opacity.reshape(P, 1), width.reshape(P, 1)), dim=1).to(torch.float32).contiguous()


# ---- numpy path ------------------------------------------------------------------------------------------------------------------
_BUDGET = 1 << 21          # elements of one vectorised block (strands x padded segments, or strands x points)


def _check_tables(offsets, rows, seg, n_ep, P):
    total = rows.shape[0]
    if offsets[0] != 0 or offsets[-1] != total or np.any(offsets[1:] < offsets[:-1]) or seg.shape[0] != total:
        raise ValueError("strand tables: offsets do not describe the rows")
    if total and (rows.min() < 0 or rows.max() >= n_ep):
        raise ValueError("strand tables: rows name endpoint ids outside the endpoint table")
    if total and (seg.min() < 0 or seg.max() >= P):
        raise ValueError("strand tables: segment rows outside the attribute table")


def _segment_lengths(ep, rows):
    d = ep[rows[:, 1]].astype(np.float64) - ep[rows[:, 0]].astype(np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def arclen_numpy(offsets, rows, ep):
    """(cum [total + S], length [S]): cum[offsets[s] + s + i] = cum_i of strand s, summed in segment order (np.cumsum along the rows of
    a zero-padded [strands, segments] block: strands of similar length share a block)."""
    S, total = len(offsets) - 1, rows.shape[0]
    seglen = _segment_lengths(ep, rows)
    n = offsets[1:] - offsets[:-1]
    cum = np.zeros(total + S, np.float64)
    order = np.argsort(n, kind="stable")
    n_sorted = n[order]
    pos = 0
    while pos < S:
        take = int(max(1, min(S - pos, 4096, _BUDGET // max(1, int(n_sorted[min(S - 1, pos + 4095)])))))
        sel = order[pos:pos + take]
        pos += take
        nn = n[sel]
        width = int(nn.max())
        if width == 0:
            continue
        j = np.arange(width)
        valid = j[None, :] < nn[:, None]
        src = np.where(valid, offsets[sel][:, None] + j[None, :], 0)
        run = np.cumsum(np.where(valid, seglen[src], 0.0), axis=1)
        dst = (offsets[sel] + sel)[:, None] + 1 + j[None, :]
        cum[dst[valid]] = run[valid]
    return cum, cum[offsets[1:] + np.arange(S)]


def _vertex_ids(rows, o0, n, i):
    """Endpoint id of joint i (0..n) of the strands starting at rows o0 with n segments (arrays of one shape)."""
    last = i >= n
    return np.where(last, rows[o0 + n - 1, 1], rows[o0 + np.minimum(i, n - 1), 0])


def _joint_attrs(attr64, seg, o0, n, i):
    """a_i [.., C]: the mean of the two segments that meet at joint i; at the ends both are the end segment (0.5 (x + x) = x)."""
    prev, cur = seg[o0 + np.clip(i - 1, 0, n - 1)], seg[o0 + np.clip(i, 0, n - 1)]
    return 0.5 * (attr64[prev] + attr64[cur])


def resample_numpy(offsets, rows, seg, ep, attr, cum, kept, M):
    """points [K M, 3], attrs [K M, C] (float32) of the kept strands; M = 0: the joints (out_offsets = prefix sums of n + 1)."""
    C = attr.shape[1]
    attr64 = attr.astype(np.float64)
    n_all = offsets[1:] - offsets[:-1]
    K = kept.shape[0]
    if M == 0:
        cnt = n_all[kept] + 1
        out_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        k = np.repeat(np.arange(K), cnt)
        i = np.arange(out_off[-1]) - out_off[k]
        o0, n = offsets[kept][k], n_all[kept][k]
        pts = ep[_vertex_ids(rows, o0, n, i)] if out_off[-1] else np.zeros((0, 3), np.float32)
        att = _joint_attrs(attr64, seg, o0, n, i).astype(np.float32) if out_off[-1] else np.zeros((0, C), np.float32)
        return np.ascontiguousarray(pts, np.float32), att, out_off
    pts, att = np.empty((K, M, 3), np.float32), np.empty((K, M, C), np.float32)
    frac = np.arange(M, dtype=np.float64) / np.float64(M - 1)
    step = max(1, _BUDGET // (M * max(3, C)))
    for b in range(0, K, step):
        ks = kept[b:b + step]
        o0, n = offsets[ks][:, None], n_all[ks][:, None]
        base = o0 + ks[:, None]
        t = frac[None, :] * cum[base + n]
        lo, hi = np.zeros(t.shape, np.int64), np.broadcast_to(n + 1, t.shape).copy()
        while True:                                    # largest i with cum_i <= t
            act = hi - lo > 1
            if not act.any():
                break
            mid = (lo + hi) >> 1
            le = cum[base + mid] <= t
            lo, hi = np.where(act & le, mid, lo), np.where(act & ~le, mid, hi)
        i = np.minimum(lo, n - 1)
        va, vb = ep[_vertex_ids(rows, o0, n, i)].astype(np.float64), ep[_vertex_ids(rows, o0, n, i + 1)].astype(np.float64)
        d = vb - va
        seglen = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        w = np.divide(t - cum[base + i], seglen, out=np.zeros_like(t), where=seglen > 0)
        a0 = _joint_attrs(attr64, seg, o0, n, i)
        p = (va + w[..., None] * d).astype(np.float32)
        a = (a0 + w[..., None] * (_joint_attrs(attr64, seg, o0, n, i + 1) - a0)).astype(np.float32)
        zero, tip = np.zeros_like(n[:, 0]), n[:, 0]
        for col, at in ((0, zero), (M - 1, tip)):      # the end samples are the end joints themselves
            p[:, col] = ep[_vertex_ids(rows, o0[:, 0], tip, at)]
            a[:, col] = _joint_attrs(attr64, seg, o0[:, 0], tip, at).astype(np.float32)
        pts[b:b + step], att[b:b + step] = p, a
    return pts.reshape(K * M, 3), att.reshape(K * M, C), np.arange(K + 1, dtype=np.int64) * M


# ---- device path -----------------------------------------------------------------------------------------------------------------
def arclen_device(offsets, rows, ep):
    """hgs_strand_arclen on device tables: (cum [total + S] float64, length [S] float64), both on the device."""
    import hgs_runtime as rt
    dev = ep.device
    S, total = int(offsets.numel()) - 1, int(rows.shape[0])
    cum = torch.empty(total + S, dtype=torch.float64, device=dev)
    length = torch.empty(S, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_strand_arclen(rt.current_stream(), S, rt.ptr(offsets), rt.ptr(rows), total, rt.ptr(ep), int(ep.shape[0]),
                                            rt.ptr(cum), rt.ptr(length), rt.ptr(status)))
    return cum, length, status


def resample_device(offsets, rows, seg, ep, attr, cum, kept, M, out_offsets=None, n_out=None):
    """hgs_strand_resample: (points [n_out, 3], attrs [n_out, C]) float32 on the device.  M >= 2: n_out = K M.  M = 0 (the joints):
    out_offsets is the [K+1] int64 device tensor of the prefix sums of n + 1, and n_out its last entry, which the caller passes
    (it knows it from the host offsets; reading it here would be a synchronisation)."""
    import hgs_runtime as rt
    dev = ep.device
    S, total, K, C = int(offsets.numel()) - 1, int(rows.shape[0]), int(kept.numel()), int(attr.shape[1])
    if M:
        n_out, dev_off = K * M, None
    else:
        if out_offsets is None or n_out is None:
            raise ValueError("resample_device: M = 0 needs out_offsets [K+1] and n_out")
        dev_off = rt.require_gpu_tensor(out_offsets, "out_offsets", torch.int64)
        if dev_off.numel() != K + 1:
            raise ValueError(f"resample_device: out_offsets has {dev_off.numel()} entries for {K} strands")
        n_out = int(n_out)
    pts = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    att = torch.empty((n_out, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_strand_resample(rt.current_stream(), S, rt.ptr(offsets), rt.ptr(rows), rt.ptr(seg), total, rt.ptr(ep),
                                              int(ep.shape[0]), rt.ptr(attr), int(attr.shape[0]), C, rt.ptr(cum), K, rt.ptr(kept), int(M),
                                              rt.ptr(dev_off), n_out, rt.ptr(pts), rt.ptr(att)))
    return pts, att


def _device_tables(model):
    """(offsets, rows, global segment rows) on the model's device: what the device walk left there, or the host tables uploaded."""
    import hgs_runtime as rt
    si = model.strands_info
    dev_tables = getattr(model, "_strands_dev", None)
    if dev_tables is not None and dev_tables[0].numel() == len(si.offsets) and dev_tables[1].shape[0] == len(si.rows):
        off, rows, seg = dev_tables
    else:
        dev = model._endpoints.device
        off = torch.as_tensor(np.asarray(si.offsets, np.int64), device=dev)
        rows = torch.as_tensor(np.asarray(si.rows, np.int64).reshape(-1, 2), device=dev)
        seg = torch.as_tensor(np.asarray(model._strand_global_rows(), np.int64), device=dev)
    return tuple(rt.require_gpu_tensor(t, "strand table", torch.int64) for t in (off, rows.reshape(-1, 2), seg))


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def _root_distance(model, v0):
    from scene.hair_gaussian_model import nearest_distance
    roots = None if model.ref_strand_root is None else np.asarray(model.ref_strand_root)
    if roots is None or roots.shape[0] == 0:
        raise ValueError("max_root_distance needs the capture's strand roots (model.ref_strand_root is empty)")
    return nearest_distance(v0, torch.as_tensor(roots.reshape(-1, 3), device=v0.device)).cpu().numpy()


def resample_strands(model, points=100, min_segments=1, min_length=0.0, max_root_distance=None, device=None):
    """The strands of `model` (HairGaussianModel) as `points` points each by arc length (0: their joints), see the module docstring.
    Returns a StrandExport of host arrays.  device=None: numpy; "cuda": the HIP kernels (the model must live on the GPU)."""
    M = int(points)
    if M < 0 or M == 1:
        raise ValueError(f"points = {points}: 0 for the joints themselves, else at least 2 points per strand")
    if model.strands_info is None:
        model.compute_strands_info()
    si = model.strands_info
    offsets = np.asarray(si.offsets, np.int64)
    S = len(offsets) - 1
    n = offsets[1:] - offsets[:-1]
    attr_t = export_attributes(model)
    ep_t = model._endpoints.detach().to(torch.float32).contiguous()
    if device is None:
        rows = np.asarray(si.rows, np.int64).reshape(-1, 2)
        seg = np.asarray(model._strand_global_rows(), np.int64) if rows.shape[0] else np.zeros(0, np.int64)
        ep, attr = ep_t.cpu().numpy(), attr_t.cpu().numpy()
        _check_tables(offsets, rows, seg, ep.shape[0], attr.shape[0])
        cum, length = arclen_numpy(offsets, rows, ep)
    else:
        import hgs_runtime as rt
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernels)")
        ep_t = rt.require_gpu_tensor(ep_t, "the model's endpoints", torch.float32)
        attr_t = rt.require_gpu_tensor(attr_t, "the attribute table", torch.float32)
        off_d, rows_d, seg_d = _device_tables(model)
        cum_d, length_d, status = arclen_device(off_d, rows_d, ep_t)
        length = length_d.cpu().numpy()
        bad = int(status.item())
        if bad:
            raise RuntimeError("resample_strands(): the strand rows name endpoint ids outside the endpoint table" if bad == 1
                               else "resample_strands(): the strand offsets do not describe the strand rows")
    keep = (n >= max(1, int(min_segments))) & (length >= float(min_length))
    if max_root_distance is not None:
        cand = np.nonzero(keep)[0]
        if device is None:
            v0 = ep_t[torch.as_tensor(rows[offsets[cand], 0], device=ep_t.device)] if cand.size else ep_t[:0]
        else:
            v0 = ep_t[rows_d[off_d[torch.as_tensor(cand, device=ep_t.device)], 0]] if cand.size else ep_t[:0]
        dist = _root_distance(model, v0)
        keep[cand[dist > float(max_root_distance)]] = False
    kept = np.nonzero(keep)[0].astype(np.int64)
    if kept.size and kept[-1] > np.iinfo(np.int32).max:
        raise ValueError("more than 2^31 strands")
    if device is None:
        pts, att, out_off = resample_numpy(offsets, rows, seg, ep, attr, cum, kept, M)
    else:
        K = kept.shape[0]
        out_off = np.arange(K + 1, dtype=np.int64) * M if M else np.concatenate([[0], np.cumsum(n[kept] + 1)]).astype(np.int64)
        kept_d = torch.as_tensor(kept.astype(np.int32), device=ep_t.device)
        native = {} if M else dict(out_offsets=torch.as_tensor(out_off, device=ep_t.device), n_out=int(out_off[-1]))
        pts_d, att_d = resample_device(off_d, rows_d, seg_d, ep_t, attr_t, cum_d, kept_d, M, **native)
        pts, att = pts_d.cpu().numpy(), att_d.cpu().numpy()
    return StrandExport(pts, att, out_off, kept, length[kept])
