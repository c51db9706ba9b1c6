"""The guide selection's contract (hair-gs_amd/scene/strand_guides.py) restated as plain Python loops: scalar float64 (Python floats),
one statement per line of the contract, no numpy arithmetic.  Slow on purpose; tests/guides_cases.py keeps the cases tiny."""
import math

import numpy as np

INF = float("inf")


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def features(points, offsets, samples):
    """(N, M, S, x, status): x[i] = the S sampled points of strand i as a flat list of 3S Python floats."""
    off = [int(v) for v in offsets]
    N = len(off) - 1
    M = off[1] - off[0] if N else 0
    assert all(off[i + 1] - off[i] == M for i in range(N)) and (N == 0 or M >= 2)
    S = min(samples, M) if N else samples
    joints = [(s * (M - 1)) // (S - 1) for s in range(S)]
    p = np.asarray(points, np.float32).astype(np.float64).tolist()                 # the float32 inputs as doubles
    x, status = [], []
    for i in range(N):
        rows = p[off[i]:off[i + 1]]
        status.append(0 if all(math.isfinite(c) for row in rows for c in row) else 1)
        x.append([c for j in joints for c in rows[j]])
    return N, M, S, x, status


def d2_of(xi, ck, S):
    acc = 0.0
    for s in range(S):
        dx = xi[3 * s] - ck[3 * s]
        dy = xi[3 * s + 1] - ck[3 * s + 1]
        dz = xi[3 * s + 2] - ck[3 * s + 2]
        acc = acc + ((dx * dx + dy * dy) + dz * dz)
    return acc


def assign(x, E, cent, S):
    """{i: (label, dist2)} for the strands E: the k smallest by (d2, k)."""
    out = {}
    for i in E:
        best_k, best_d = -1, INF
        for k, ck in enumerate(cent):
            d = d2_of(x[i], ck, S)
            if best_k < 0 or d < best_d:                                           # strict <: ties stay with the smaller k
                best_k, best_d = k, d
        out[i] = (best_k, best_d)
    return out


def update(x, E, label, cent, S):
    """The centroids after one update (a new list), and the member counts."""
    new, count = [], []
    for k, ck in enumerate(cent):
        members = [i for i in E if label[i][0] == k]                               # ascending strand index
        count.append(len(members))
        if not members:
            new.append(list(ck))
            continue
        row = []
        for c in range(3 * S):
            acc = 0.0
            for i in members:
                acc = acc + x[i][c]
            row.append(acc / float(len(members)))
        new.append(row)
    return new, count


def pick(E, label, K):
    guide, count = [], []
    for k in range(K):
        members = [i for i in E if label[i][0] == k]
        count.append(len(members))
        best = -1
        for i in members:
            if best < 0 or label[i][1] < label[best][1]:                           # ascending i and strict <: ties stay with the smaller i
                best = i
        guide.append(best)
    return guide, count


def guides(points, offsets, k, samples=16, iters=10, trace=None):
    """(labels int32 [N], dist2 float64 [N], guide int64 [K], count int32 [K], status int32 [N], iterations, converged, centroids
    float64 [K, S, 3], first_dist2 float64 [N]).  trace (a list): appended (centroids, labels, dist2) of every assignment."""
    N, M, S, x, status = features(points, offsets, samples)
    E = [i for i in range(N) if status[i] == 0]
    n_E = len(E)
    K = min(k, n_E)
    labels, dist2, first = [-1] * N, [INF] * N, [INF] * N
    cent, guide, count, t, converged = [], [], [], 0, False
    if K > 0:
        cent = [list(x[E[((2 * q + 1) * n_E) // (2 * K)]]) for q in range(K)]
        label = prev = None
        while t < iters:
            if t > 0:
                cent, _ = update(x, E, label, cent, S)
            prev = label
            label = assign(x, E, cent, S)
            t += 1
            if trace is not None:
                trace.append(([list(c) for c in cent], dict(label)))
            if t == 1:
                for i in E:
                    first[i] = label[i][1]
            elif all(label[i][0] == prev[i][0] for i in E):
                converged = True
                break
        for i in E:
            labels[i], dist2[i] = label[i]
        guide, count = pick(E, label, K)
    return (np.array(labels, np.int32).reshape(N), np.array(dist2, np.float64).reshape(N), np.array(guide, np.int64).reshape(K),
            np.array(count, np.int32).reshape(K), np.array(status, np.int32).reshape(N), t, converged,
            np.array(cent, np.float64).reshape(K, S, 3), np.array(first, np.float64).reshape(N))
