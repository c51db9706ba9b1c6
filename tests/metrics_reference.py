"""Brute-force statements of the strand-metric kernels (include/hgs.h, hgs_oriented_match / hgs_strand_votes): plain numpy in
float64, every (A point, B point) pair decided by the header's two tests in the header's order of operations, no tree in the
decision.  Everything returned is an integer, so every comparison against these functions is for equality."""
import numpy as np


def pair_bits(a_pts, a_dirs, b_pts, b_dirs, thresholds, bidirectional):
    """uint32 [nA][nB]: bit k set iff B point j matches A point i under pair k = thresholds[k] = (r_k, cos_k):
    d2 = (dx*dx + dy*dy) + dz*dz <= r_k*r_k and dot = (ux*vx + uy*vy) + uz*vz >= cos_k (|dot| when bidirectional).
    A comparison with a NaN is False, so a NaN never matches."""
    a_pts, a_dirs = np.asarray(a_pts, np.float64).reshape(-1, 3), np.asarray(a_dirs, np.float64).reshape(-1, 3)
    b_pts, b_dirs = np.asarray(b_pts, np.float64).reshape(-1, 3), np.asarray(b_dirs, np.float64).reshape(-1, 3)
    thr = np.asarray(thresholds, np.float64).reshape(-1, 2)
    assert 1 <= len(thr) <= 32
    with np.errstate(invalid="ignore", over="ignore"):
        dx = b_pts[None, :, 0] - a_pts[:, None, 0]
        dy = b_pts[None, :, 1] - a_pts[:, None, 1]
        dz = b_pts[None, :, 2] - a_pts[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        bits = np.zeros(d2.shape, np.uint32)
        i, j = np.nonzero(d2 <= (thr[:, 0] * thr[:, 0]).max())      # (a pair outside the largest r_k*r_k fails every first test)
        d2, u, v = d2[i, j], a_dirs[i], b_dirs[j]
        dot = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
        if bidirectional:
            dot = np.abs(dot)
        m = np.zeros(len(i), np.uint32)
        for k, (r, c) in enumerate(thr):
            m |= ((d2 <= r * r) & (dot >= c)).astype(np.uint32) << np.uint32(k)
        bits[i, j] = m
    return bits


def match_masks(a_pts, a_dirs, b_pts, b_dirs, thresholds, bidirectional, pruned=False, chunk=512):
    """uint32 [nA]: bit k set iff some B point matches A point i under pair k (pair_bits).  In chunks over A.
    pruned=True (for large B only): the candidates of a point come from a cKDTree ball query of radius r_max (1 + 1e-9);
    each candidate still gets the exact test, the tree only leaves out points that are too far to pass it."""
    a_pts, a_dirs = np.asarray(a_pts, np.float64).reshape(-1, 3), np.asarray(a_dirs, np.float64).reshape(-1, 3)
    b_pts, b_dirs = np.asarray(b_pts, np.float64).reshape(-1, 3), np.asarray(b_dirs, np.float64).reshape(-1, 3)
    out = np.zeros(len(a_pts), np.uint32)
    if len(b_pts) == 0 or len(a_pts) == 0:
        return out
    if pruned:
        from scipy.spatial import cKDTree
        assert np.isfinite(a_pts).all() and np.isfinite(b_pts).all()
        rmax = float(np.asarray(thresholds, np.float64).reshape(-1, 2)[:, 0].max())
        lists = cKDTree(b_pts).query_ball_point(a_pts, rmax * (1 + 1e-9))
        for i, js in enumerate(lists):
            if js:
                out[i] = np.bitwise_or.reduce(pair_bits(a_pts[i:i + 1], a_dirs[i:i + 1], b_pts[js], b_dirs[js], thresholds, bidirectional), axis=1)[0]
        return out
    for i0 in range(0, len(a_pts), chunk):
        s = slice(i0, i0 + chunk)
        out[s] = np.bitwise_or.reduce(pair_bits(a_pts[s], a_dirs[s], b_pts, b_dirs, thresholds, bidirectional), axis=1)
    return out


def strand_votes(a_pts, a_dirs, offsets, b_pts, b_dirs, b_strand, thresholds, bidirectional):
    """(best int64 [K][S], entries int64 [S]) of A's S strands (runs offsets[s] .. offsets[s+1] of its points).
    best[k][s]: over the distinct (point of s, B strand) matches under pair k, the points per B strand, the largest count.
    entries[s]: the distinct (point, B strand) pairs that match under at least one pair -- what a vote table has to hold."""
    a_pts, a_dirs = np.asarray(a_pts, np.float64).reshape(-1, 3), np.asarray(a_dirs, np.float64).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    K, S = len(np.asarray(thresholds).reshape(-1, 2)), len(offsets) - 1
    best, entries = np.zeros((K, S), np.int64), np.zeros(S, np.int64)
    if len(np.asarray(b_pts).reshape(-1, 3)) == 0:
        return best, entries
    ids, inv = np.unique(np.asarray(b_strand).astype(np.int64), return_inverse=True)    # (only equality matters)
    inv = inv.reshape(-1)
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if hi == lo:
            continue
        votes = np.zeros((hi - lo, len(ids)), np.uint32)          # per (point, B strand): the pairs under which it matched
        for i0 in range(lo, hi, 256):
            i1 = min(i0 + 256, hi)
            bits = pair_bits(a_pts[i0:i1], a_dirs[i0:i1], b_pts, b_dirs, thresholds, bidirectional)
            li, j = np.nonzero(bits)
            np.bitwise_or.at(votes, (li + (i0 - lo), inv[j]), bits[li, j])
        entries[s] = np.count_nonzero(votes)
        for k in range(K):
            best[k, s] = ((votes >> np.uint32(k)) & np.uint32(1)).sum(0, dtype=np.int64).max()
    return best, entries


def counts(mask, K):
    """Matched points per pair from a uint32 mask array."""
    mask = np.asarray(mask, np.uint32)
    return [int(np.count_nonzero(mask & np.uint32(1 << k))) for k in range(K)]


def metrics_from_counts(precision_counts, n_pred, recall_counts, n_gt, best=None, sizes=None, bidirectional=False):
    """The metric dict from integers, by the host arithmetic both backends of loss/metrics.py share (_ratio, _consistency,
    _assemble): precision_counts[k] matched points of the prediction, recall_counts[k] of the ground truth, best[k][s] and
    sizes[s] of the ground truth's strands in ascending id order (None: no strand consistency)."""
    from loss.metrics import _assemble, _consistency, _ratio
    K = len(precision_counts)
    out = {"precision": {}, "recall": {}, "f1": {}, "strand_consistency": {}}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(K):
            out["precision"][k] = _ratio(precision_counts[k], n_pred)
            out["recall"][k] = _ratio(recall_counts[k], n_gt)
            if best is not None:
                out["strand_consistency"][k] = _consistency(best[k], sizes)
    return _assemble(out, K, bidirectional)


def reference_metrics(pred, gt, dist_ths, angle_ths, bidirectional):
    """compute_metrics(pred, gt) from the brute-force integers alone (pred, gt: anything with points, directions and
    points_id_to_strand_id).  Pairs beyond 32 go through a second pass, as in the GPU path."""
    thr = np.stack([np.asarray(dist_ths, np.float64), np.cos(np.deg2rad(np.asarray(angle_ths, np.float64)))], 1)
    gt_ids = np.asarray(gt.points_id_to_strand_id)
    _, inv, sizes = np.unique(gt_ids, return_inverse=True, return_counts=True)
    order = np.argsort(inv.reshape(-1), kind="stable")
    gp, gd = np.asarray(gt.points, np.float64)[order], np.asarray(gt.directions, np.float64)[order]
    pp, pd = np.asarray(pred.points, np.float64), np.asarray(pred.directions, np.float64)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    pc, rc, best = [], [], []
    for k0 in range(0, len(thr), 32):
        t = thr[k0:k0 + 32]
        pc += counts(match_masks(pp, pd, gp, gd, t, bidirectional), len(t))
        rc += counts(match_masks(gp, gd, pp, pd, t, bidirectional), len(t))
        best.append(strand_votes(gp, gd, offsets, pp, pd, pred.points_id_to_strand_id, t, bidirectional)[0])
    return metrics_from_counts(pc, len(pp), rc, len(gp), np.concatenate(best, 0), sizes, bidirectional)
