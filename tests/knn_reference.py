"""Brute-force references of the neighbour searches (csrc/hgs_knn.hip), plain numpy, nothing from the product package.

Every float32 reference evaluates the kernel's own expression operation by operation (numpy rounds each float32 operation
once: no contraction), so a kernel that is exact has the same BITS; the float64 forms are the same expressions on the float32
inputs widened.  How far the two may be apart (u = 2^-24, no term subnormal):

  d2 = (dx dx + dy dy) + dz dz: every rounding is a factor (1 + e), |e| <= u, and every term is >= 0, so the factors never
  cancel.  A rounded difference enters its product twice (2 factors), the product is rounded (3), and a term passes through at
  most two sums (5): |d2_32 - d2_64| <= ((1 + u)^5 - 1) d2_64 <= 6 u d2_64.
  The k-th smallest of values that are each within a factor (1 +- delta) of the true ones is within that factor of the true k-th
  smallest (at least k of the approximate values are <= (1 + delta) x the true k-th, and at most k - 1 are < (1 - delta) x it):
  the bar holds for every column of the 3-NN although the two precisions may pick different neighbours.
  mean = ((b0 + b1) + b2) / 3: two more sums and a division, 8 roundings: |mean_32 - mean_64| <= 9 u mean_64.
  Both are exactly 0 where the float64 value is 0."""
import numpy as np

U = 2.0 ** -24
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _quiet():
    return np.errstate(invalid="ignore", over="ignore", under="ignore")


def _dist2_rows(p, s, e):
    """[e - s, P] squared distances of the rows s..e to every point, in p's precision: (dx dx + dy dy) + dz dz."""
    dx = p[s:e, None, 0] - p[None, :, 0]
    dy = p[s:e, None, 1] - p[None, :, 1]
    dz = p[s:e, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _brute_dist2(p, chunk):
    P = p.shape[0]
    big = p.dtype.type(FLT_MAX)
    out = np.empty(P, p.dtype)
    with _quiet():
        for s in range(0, P, chunk):
            e = min(P, s + chunk)
            d = _dist2_rows(p, s, e)
            d[np.arange(e - s), np.arange(s, e)] = big           # the point itself is excluded by index
            d = np.where(d < big, d, big)                        # (a candidate enters only while it is < the FLT_MAX start)
            if P < 4:
                d = np.concatenate([d, np.full((e - s, 3), big, p.dtype)], axis=1)
            b = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
            t = (b[:, 0] + b[:, 1]) + b[:, 2]
            t = np.where(t > big, p.dtype.type(np.inf), t)       # (float64: what overflows in float32 is +inf there too)
            out[s:e] = t / p.dtype.type(3)
    return out


def brute_dist2_f32(p, chunk=256):
    """distCUDA2's contract: mean of the three smallest squared distances to OTHER points, float32 (oracle/knn_oracle.c without
    the pruning).  Fewer than three comparable neighbours leave FLT_MAX terms, whose sum overflows to +inf."""
    p = np.ascontiguousarray(p, np.float32)
    assert p.dtype == np.float32
    return _brute_dist2(p, chunk)


def brute_dist2_f64(p, chunk=256):
    return _brute_dist2(np.ascontiguousarray(p, np.float32).astype(np.float64), chunk)


def _brute_knn3(p, chunk):
    n = p.shape[0]
    inf = p.dtype.type(np.inf)
    d2 = np.full((n, 3), inf, p.dtype)
    idx = np.full((n, 3), -1, np.int64)
    k = min(3, n)
    with _quiet():
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            dx = p[s:e, None, 0] - p[None, :, 0]
            dy = p[s:e, None, 1] - p[None, :, 1]
            dz = p[s:e, None, 2] - p[None, :, 2]
            d = dx * dx + dy * dy + dz * dz                      # left to right, the point itself included
            d = np.where(d < inf, d, inf)                        # NaN and +inf compare smaller than nothing
            order = np.argsort(d, axis=1, kind="stable")[:, :k]  # (distance, index)
            v = np.take_along_axis(d, order, axis=1)
            d2[s:e, :k] = v
            idx[s:e, :k] = np.where(v < inf, order, -1)
    return d2, idx


def brute_knn3_f32(p, chunk=256):
    """hgs_knn3's contract: (squared distances [n, 3], indices [n, 3]) of the three nearest points of the set, the point itself
    included, ordered by (distance, index); fewer than three comparable candidates: index -1, distance +inf."""
    return _brute_knn3(np.ascontiguousarray(p, np.float32), chunk)


def brute_knn3_f64(p, chunk=256):
    return _brute_knn3(np.ascontiguousarray(p, np.float32).astype(np.float64), chunk)


def brute_pairs_f32(pos, dirs, r, min_cos, bidir):
    """hgs_radius_pairs' statement in float32: the pairs (a, b), a < b, with d2 <= r2 and dot >= min_cos.  Returns
    (pairs int64 [K, 2] in lexicographic order, float32 sqrt(d2) [K])."""
    pos = np.ascontiguousarray(pos, np.float32)
    dirs = np.ascontiguousarray(dirs, np.float32)
    r2 = np.float32(r) * np.float32(r)
    mc = np.float32(min_cos)
    n = pos.shape[0]
    A, B, D = [], [], []
    with _quiet():
        for s in range(0, n, 512):
            e = min(n, s + 512)
            dx = pos[None, :, 0] - pos[s:e, None, 0]
            dy = pos[None, :, 1] - pos[s:e, None, 1]
            dz = pos[None, :, 2] - pos[s:e, None, 2]
            d2 = dx * dx + dy * dy + dz * dz
            dot = -(dirs[s:e, None, 0] * dirs[None, :, 0] + dirs[s:e, None, 1] * dirs[None, :, 1]
                    + dirs[s:e, None, 2] * dirs[None, :, 2])
            if bidir:
                dot = np.abs(dot)
            keep = (d2 <= r2) & (dot >= mc) & (np.arange(n)[None, :] > np.arange(s, e)[:, None])
            a, b = np.nonzero(keep)
            A.append(a + s)
            B.append(b)
            D.append(np.sqrt(d2[a, b]))
    if not A:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.float32)
    return np.stack([np.concatenate(A), np.concatenate(B)], 1).astype(np.int64), np.concatenate(D).astype(np.float32)


def kdtree_pairs(pos, dirs, r, min_cos, bidir):
    """The CPU model's statement: scipy cKDTree.query_pairs on the float64 positions, then the direction test in float32."""
    from scipy.spatial import cKDTree
    pos = np.ascontiguousarray(pos, np.float32)
    dirs = np.ascontiguousarray(dirs, np.float32)
    if pos.shape[0] < 2:
        return np.zeros((0, 2), np.int64)
    ref = cKDTree(pos.astype(np.float64)).query_pairs(r=r, output_type="ndarray").astype(np.int64).reshape(-1, 2)
    dot = -(dirs[ref[:, 0]] * dirs[ref[:, 1]]).sum(1)
    dot = np.abs(dot) if bidir else dot
    return ref[dot >= min_cos]


def pairs_excused(pos, dirs, r, min_cos, pairs):
    """The excuse of tests/test_gpu_knn.py, per row of `pairs` [K, 2]: the pair sits within 1e-6 of the radius or within 1e-5 of
    the cosine (float64 on the float32 inputs)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    p, u = np.asarray(pos, np.float32).astype(np.float64), np.asarray(dirs, np.float32).astype(np.float64)
    d = np.linalg.norm(p[pairs[:, 0]] - p[pairs[:, 1]], axis=1)
    c = -(u[pairs[:, 0]] * u[pairs[:, 1]]).sum(axis=1)
    return (np.abs(d - r) < 1e-6) | (np.abs(np.abs(c) - min_cos) < 1e-5)


def brute_nearest_f64(pts, refs, chunk=4096):
    """hgs_nearest_distance_f64's statement: sqrt((dx dx + dy dy) + dz dz) to the nearest reference, float64."""
    p = np.asarray(pts).astype(np.float64)
    refs = np.asarray(refs, np.float64)
    out = np.empty(p.shape[0], np.float64)
    for s in range(0, p.shape[0], chunk):
        d = p[s:s + chunk, None, :] - refs[None, :, :]
        out[s:s + chunk] = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1))
    return out


def within(a32, a64, k):
    """|a32 - a64| <= k u a64 element-wise, exactly 0 where a64 is 0; +inf matches +inf."""
    a32 = np.asarray(a32, np.float64)
    a64 = np.asarray(a64, np.float64)
    both_inf = np.isposinf(a32) & np.isposinf(a64)
    with _quiet():
        ok = np.abs(a32 - a64) <= k * U * a64
    return ok | both_inf
