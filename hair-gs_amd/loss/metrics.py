"""Strand-reconstruction metrics (counterpart of the reference's loss/metrics.py:12-173): precision / recall / F1 of
oriented points under (distance, angle) thresholds and strand consistency.  Two backends behind compute_metrics(device=):
  * CPU (default, scipy cKDTree).  Instead of the reference's Python loop over every point, the radius-query result is
    flattened to CSR arrays and reduced with numpy; the threshold pairs run on a thread pool (cKDTree releases the GIL)
    instead of 8 forked processes with a Manager dict.
  * GPU (csrc/hgs_metrics.hip): one pass per direction tests every threshold pair (per-point bitmasks), and one workgroup
    per strand counts the consistency votes.  Both backends hand integer counts to the same host arithmetic (_ratio,
    _consistency, _assemble), so the dicts are equal bit for bit wherever the per-point matches agree.  (The GPU path
    takes every dot product in float64; the CPU path's einsum does too unless BOTH sides' directions are float32.)"""
import warnings
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Optional

import numpy as np
from scipy.spatial import cKDTree


@dataclass
class HairEvalData:
    """Oriented point cloud: points [N,3], unit directions [N,3], optional strand id per point, optional edges between points
    (reference data/eval_data.py:16-20)."""
    points: np.ndarray
    directions: np.ndarray
    points_id_to_strand_id: Optional[np.ndarray] = None
    edges: Optional[np.ndarray] = None


def _csr_matches(p1, p2, dist_th, cos_th, bidirectional):
    """For every point of p1: p2 indices within dist_th whose direction agrees.  Returns (row_of_match, p2_index)."""
    lists = cKDTree(p2.points).query_ball_point(p1.points, r=dist_th, workers=-1)
    lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
    if lens.sum() == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    rows = np.repeat(np.arange(len(lists)), lens)
    cols = np.fromiter((j for x in lists for j in x), dtype=np.int64, count=int(lens.sum()))
    dot = np.einsum("ij,ij->i", p1.directions[rows], p2.directions[cols])
    if bidirectional:
        dot = np.abs(dot)
    keep = dot >= cos_th
    return rows[keep], cols[keep]


def pct_matched_points(p1, p2, dist_th, angle_th, bidirectional=False, compute_strand_consistency=False):
    """Fraction of p1's points that have a p2 point within dist_th with direction within angle_th; optionally the
    strand consistency: per p1 strand, the largest share of its points matched to one p2 strand, averaged
    (reference :12-85).  Returns (ratio, strand_consistency or None)."""
    cos_th = np.cos(np.deg2rad(angle_th))
    n = p1.points.shape[0]
    rows, cols = _csr_matches(p1, p2, dist_th, cos_th, bidirectional)
    matched = np.zeros(n, bool)
    matched[rows] = True
    ratio = _ratio(matched.sum(), n)
    consistency = None
    if compute_strand_consistency:
        s1 = p1.points_id_to_strand_id
        s2 = p2.points_id_to_strand_id
        strands, n_pts = np.unique(s1, return_counts=True)
        # each p1 point votes once for every distinct p2 strand it matched
        votes = np.unique(np.stack([rows, s2[cols]], 1), axis=0) if rows.size else np.zeros((0, 2), np.int64)
        best = np.zeros(len(strands), np.int64)
        if votes.shape[0]:
            key = np.stack([s1[votes[:, 0]], votes[:, 1]], 1)          # (p1 strand, p2 strand)
            uk, cnt = np.unique(key, axis=0, return_counts=True)
            np.maximum.at(best, np.searchsorted(strands, uk[:, 0]), cnt)
        consistency = _consistency(best, n_pts)
    return ratio, consistency


# ---- the host arithmetic both backends share: integer counts -> the ratios the reference reports ----
def _ratio(matched, n):
    """matched points (an integer) / n: a numpy float64 (nan for n == 0, as numpy divides)."""
    return np.int64(matched) / n


def _consistency(best, sizes):
    """Strand consistency from best[s] = the most points of strand s that one strand of the other side matched, and sizes[s] =
    its point count, strands in ascending id order: sum(best / size) over the strands with a vote, in that order, divided by the
    strand count (ZeroDivisionError without strands, like the reference)."""
    best, sizes = np.asarray(best, np.int64), np.asarray(sizes, np.int64)
    voted = best > 0
    total = sum(c / s for c, s in zip(best[voted], sizes[voted].tolist())) if voted.any() else 0.0
    return total / len(sizes)


def _assemble(out, n_pairs, bidirectional):
    """{metric: {pair index: value}} -> the reference's {metric[(b)]: array over thresholds}, with F1 from precision and recall."""
    if "f1" in out and "precision" in out and "recall" in out:
        for i in range(n_pairs):
            p, r = out["precision"].get(i), out["recall"].get(i)
            if p is not None and r is not None:
                out["f1"][i] = 2 * p * r / (p + r) if p + r > 0 else 0
    suffix = "(b)" if bidirectional else ""
    return {k + suffix: np.array([v[i] for i in range(n_pairs) if i in v]) for k, v in out.items()}


def compute_metrics(pred, gt, dist_ths=(2e-3, 3e-3, 4e-3, 4e-3), angle_ths=(20, 30, 40, 90),
                    metrics=("precision", "recall", "f1", "strand_consistency"), bidirectional=False, processes=None,
                    device=None, vote_capacity=None):
    """Returns ({metric[(b)]: array over thresholds}, [threshold labels]) like the reference (:88-173).

    device None (or a CPU device): the CPU path below.  A CUDA device: the HIP kernels of csrc/hgs_metrics.hip; the same dict,
    bit for bit, wherever the per-point matches agree (see oriented_match).  There is no fallback: without a GPU it raises
    HgsError.  vote_capacity: LDS entries of the strand-vote tables (GPU path; a power of two, default VOTE_CAPACITY)."""
    consistency = ("strand_consistency" in metrics and pred.points_id_to_strand_id is not None
                   and gt.points_id_to_strand_id is not None)
    labels = [f"{d}m&{a}°" for d, a in zip(dist_ths, angle_ths)]
    if device is not None and str(device) != "cpu":
        out = _metrics_gpu(pred, gt, dist_ths, angle_ths, metrics, bidirectional, consistency, device,
                           VOTE_CAPACITY if vote_capacity is None else vote_capacity)
        return _assemble(out, len(labels), bidirectional), labels
    jobs = []
    if "precision" in metrics:
        jobs += [("precision", i, pred, gt, d, a, False) for i, (d, a) in enumerate(zip(dist_ths, angle_ths))]
    if "recall" in metrics:
        jobs += [("recall", i, gt, pred, d, a, consistency) for i, (d, a) in enumerate(zip(dist_ths, angle_ths))]
    out = {m: {} for m in metrics}
    with ThreadPoolExecutor(max_workers=8 if processes is None else processes) as pool:
        futs = [(name, i, pool.submit(pct_matched_points, a, b, d, ang, bidirectional, cs))
                for name, i, a, b, d, ang, cs in jobs]
        for name, i, f in futs:
            ratio, cons = f.result()
            out[name][i] = ratio
            if cons is not None:
                out["strand_consistency"][i] = cons
    return _assemble(out, len(labels), bidirectional), labels


# ---- GPU path (csrc/hgs_metrics.hip through include/hgs.h hgs_oriented_match / hgs_strand_votes) ----
MAX_PAIRS = 32            # threshold pairs per kernel pass (bits of the per-point mask)
VOTE_CAPACITY = 2048      # largest LDS table of hgs_strand_votes


def _gpu_device(device):
    import torch
    import hgs_runtime as rt
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise rt.HgsError(f"strand metrics on device {device!r}: libhgs.so only runs on the GPU, there is no CPU fallback "
                          "(device=None selects the CPU path)")
    return dev


def _box(points):
    """Per-axis min and max of the finite coordinates (a NaN point never matches and may lie anywhere)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # (an axis without a finite value: all-NaN slice)
        finite = np.where(np.isfinite(points), points, np.nan)
        lo, hi = np.nanmin(finite, 0), np.nanmax(finite, 0)
    return np.ascontiguousarray(np.nan_to_num(np.concatenate([lo, hi]), nan=0.0), np.float64)


class _GpuSide:
    """One point set uploaded as float64 (float32 input widens exactly), optionally reordered."""

    def __init__(self, data, dev, order=None):
        import torch
        p, d = np.asarray(data.points, np.float64), np.asarray(data.directions, np.float64)
        if order is not None:
            p, d = p[order], d[order]
        self.n = p.shape[0]
        self.host_points, self.host_dirs = p, d
        self.points = torch.from_numpy(np.ascontiguousarray(p.reshape(-1, 3))).to(dev)
        self.dirs = torch.from_numpy(np.ascontiguousarray(d.reshape(-1, 3))).to(dev)
        self.box = _box(p.reshape(-1, 3)) if self.n else np.zeros(6)


def _match_pass(A, B, pairs, bidirectional, dev):
    """hgs_oriented_match of A against B for <= MAX_PAIRS (r, cos) pairs: (uint32 mask tensor [nA], scratch, thresholds)."""
    import torch
    import hgs_runtime as rt
    L = rt.lib()
    thr = np.ascontiguousarray(np.asarray(pairs, np.float64).reshape(-1, 2))
    mask = torch.empty(A.n, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(L.hgs_oriented_match_scratch_bytes(B.n)), dtype=torch.uint8, device=dev)
    rt.check(L.hgs_oriented_match(rt.current_stream(), A.n, B.n, len(pairs), rt.ptr(A.points), rt.ptr(A.dirs), rt.ptr(B.points),
                                  rt.ptr(B.dirs), thr.ctypes.data, int(bool(bidirectional)), B.box.ctypes.data, rt.ptr(mask),
                                  rt.ptr(scratch), scratch.numel()))
    return mask, scratch, thr


def oriented_match(a, b, dist_ths, cos_ths, bidirectional=False, device="cuda"):
    """Per point of `a` (HairEvalData): a uint32 bitmask, bit k set iff some point of `b` lies within dist_ths[k] -- decided as
    d2 = (dx*dx + dy*dy) + dz*dz <= r*r in float64, the form cKDTree.query_ball_point decides by -- with direction
    dot >= cos_ths[k] (|dot| if bidirectional).  At most MAX_PAIRS pairs.  What the metrics of the GPU path count."""
    import torch
    dev = _gpu_device(device)
    pairs = [(float(d), float(c)) for d, c in zip(dist_ths, cos_ths)]
    if not 1 <= len(pairs) <= MAX_PAIRS:
        raise ValueError(f"oriented_match: 1 .. {MAX_PAIRS} threshold pairs, got {len(pairs)}")
    with torch.cuda.device(dev):
        A, B = _GpuSide(a, dev), _GpuSide(b, dev)
        if A.n == 0:
            return np.zeros(0, np.uint32)
        mask, _, _ = _match_pass(A, B, pairs, bidirectional, dev)
        return mask.cpu().numpy().view(np.uint32)


def _counts(mask, K):
    m = mask.cpu().numpy().view(np.uint32)
    return [np.count_nonzero(m & np.uint32(1 << k)) for k in range(K)]


def _host_best(A, lo, hi, B, b_strand, pair, bidirectional):
    """The vote count of one strand (A's points lo..hi) under one pair, on the host: for strands the LDS tables cannot hold."""
    sub = HairEvalData(A.host_points[lo:hi], A.host_dirs[lo:hi])
    rows, cols = _csr_matches(sub, HairEvalData(B.host_points, B.host_dirs), pair[0], pair[1], bidirectional)
    if rows.size == 0:
        return 0
    votes = np.unique(np.stack([rows, b_strand[cols].astype(np.int64)], 1), axis=0)
    return int(np.unique(votes[:, 1], return_counts=True)[1].max())


def _metrics_gpu(pred, gt, dist_ths, angle_ths, metrics, bidirectional, consistency, device, vote_capacity):
    """{metric: {pair index: value}} of compute_metrics on the GPU: one pass per direction for up to MAX_PAIRS pairs."""
    import torch
    import hgs_runtime as rt
    dev = _gpu_device(device)
    pairs = [(float(d), float(np.cos(np.deg2rad(a)))) for d, a in zip(dist_ths, angle_ths)]   # (the CPU path's cos_th)
    chunks = [list(range(i, min(i + MAX_PAIRS, len(pairs)))) for i in range(0, len(pairs), MAX_PAIRS)]
    out = {m: {} for m in metrics}
    with torch.cuda.device(dev):
        if "precision" in metrics:
            A, B = _GpuSide(pred, dev), _GpuSide(gt, dev)
            for ch in chunks:
                counts = _counts(_match_pass(A, B, [pairs[i] for i in ch], bidirectional, dev)[0], len(ch)) if A.n else [0] * len(ch)
                for k, i in enumerate(ch):
                    out["precision"][i] = _ratio(counts[k], A.n)
        if "recall" in metrics:
            order = sizes = None
            if consistency:      # A (the GT) in strand order: CSR runs per strand, strands in ascending id order
                _, inv, sizes = np.unique(np.asarray(gt.points_id_to_strand_id), return_inverse=True, return_counts=True)
                order = np.argsort(inv.reshape(-1), kind="stable")
                offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
                b_strand_host = np.unique(np.asarray(pred.points_id_to_strand_id), return_inverse=True)[1].reshape(-1).astype(np.int32)
                b_strand = torch.from_numpy(b_strand_host).to(dev)
            A, B = _GpuSide(gt, dev, order), _GpuSide(pred, dev)
            S = 0 if sizes is None else len(sizes)
            for ch in chunks:
                K = len(ch)
                if A.n == 0:
                    counts, best = [0] * K, np.zeros((K, S), np.int64)
                else:
                    mask, scratch, thr = _match_pass(A, B, [pairs[i] for i in ch], bidirectional, dev)
                    if consistency:
                        L = rt.lib()
                        best_d = torch.zeros((K, S), dtype=torch.int32, device=dev)
                        over = torch.empty(S, dtype=torch.int32, device=dev)
                        n_over = torch.zeros(1, dtype=torch.int32, device=dev)
                        rt.check(L.hgs_strand_votes(rt.current_stream(), S, B.n, K, rt.ptr(A.points), rt.ptr(A.dirs), rt.ptr(offsets),
                                                    rt.ptr(b_strand), thr.ctypes.data, int(bool(bidirectional)), B.box.ctypes.data,
                                                    rt.ptr(scratch), int(vote_capacity), rt.ptr(best_d), rt.ptr(over), rt.ptr(n_over)))
                    counts = _counts(mask, K)
                    if consistency:
                        best = best_d.cpu().numpy().astype(np.int64)
                        off = np.concatenate([[0], np.cumsum(sizes)])
                        for s in over[:int(n_over.item())].cpu().numpy().tolist():
                            for k, i in enumerate(ch):
                                best[k, s] = _host_best(A, off[s], off[s + 1], B, b_strand_host, pairs[i], bidirectional)
                for k, i in enumerate(ch):
                    out["recall"][i] = _ratio(counts[k], A.n)
                    if consistency:
                        out["strand_consistency"][i] = _consistency(best[k], sizes)
    return out


def compute_eval_data_from_hair_gs(hair_gs, compute_edges=False, only_foreground=False):
    """Oriented points of a strand model as the reference defines them (data/eval_data.py:133-171): one point per segment of
    `strands_info.list_strands` -- its FIRST joint in strand order, root to tip --, the unit direction towards the next joint,
    and the joint's strand id.  (`strands_info` computed with only_foreground=True already holds foreground segments only;
    only_foreground=True here filters again by the current foreground mask, like the reference.)"""
    endpoints = hair_gs._endpoints.detach().cpu().numpy()
    if hair_gs.strands_info is None:          # (the constructor's default: the reference would fail here; train.evaluate() may come first)
        hair_gs.compute_strands_info(only_foreground=True)
    strands = list(hair_gs.strands_info.list_strands)
    if len(strands) == 0:                     # nothing to evaluate: an empty point set instead of np.concatenate's error
        return HairEvalData(points=np.zeros((0, 3), endpoints.dtype), directions=np.zeros((0, 3), endpoints.dtype),
                            points_id_to_strand_id=np.zeros((0,), np.int64), edges=np.zeros((0, 2), np.int32) if compute_edges else None)
    segments_id = np.concatenate(strands, axis=0)
    if only_foreground:
        mask = hair_gs.compute_foreground_mask().cpu().numpy()
        line_points = hair_gs.endpoint_pairs.cpu().numpy()[mask].flatten()
        segments_id = segments_id[np.any(np.isin(segments_id, line_points), axis=1)]
    segments = endpoints[segments_id]
    directions = segments[:, 1] - segments[:, 0]
    directions /= np.linalg.norm(directions, axis=1, keepdims=True)
    points_id = segments_id[:, 0]
    edges = None
    if compute_edges:   # indices into the new point set; single-segment strands have no edge (:160-166)
        mapping = np.zeros(segments_id.max() + 1, dtype=np.int32)
        mapping[segments_id[:, 0]] = np.arange(segments_id.shape[0])
        u, c = np.unique(segments_id, return_counts=True)
        edges = mapping[segments_id[np.isin(segments_id[:, 1], u[c > 1])]]
    return HairEvalData(points=endpoints[points_id], directions=directions,
                        points_id_to_strand_id=np.asarray(hair_gs.strands_info.id_to_strand_id)[points_id], edges=edges)


def compute_eval_data_from_gs(gaussians):
    """Oriented points of a Gaussian cloud: foreground means + the direction of the longest axis (reference
    data/eval_data.py:121-130)."""
    import torch
    with torch.no_grad():
        fg = gaussians.compute_foreground_mask()
        return HairEvalData(points=gaussians.get_xyz[fg].cpu().numpy(), directions=gaussians.get_orientation[fg].cpu().numpy())

