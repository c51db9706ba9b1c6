"""The strand deduplication restated in plain Python floats (scene/strand_dedupe.py states the contract): a double loop over the pairs
that tests every joint, then the greedy resolution in ascending index with kept_by and rounds.  It shares no code with the product and
vectorises nothing; a Python float is a double, and -, * and + round once each, so this is the contract's arithmetic operation by
operation."""
import numpy as np


def lower_lists(points, offsets, tol):
    """[[j < i with pair(i, j), ascending] for every strand i]."""
    off = [int(v) for v in offsets]
    rows = [[float(v) for v in row] for row in np.asarray(points, np.float32)]
    N = len(off) - 1
    tol2 = float(tol) * float(tol)
    lower = []
    for i in range(N):
        mine = []
        for j in range(i):
            pair = True
            for s in range(off[i + 1] - off[i]):
                a, b = rows[off[i] + s], rows[off[j] + s]
                dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
                if not ((dx * dx + dy * dy) + dz * dz <= tol2):
                    pair = False
                    break
            if pair:
                mine.append(j)
        lower.append(mine)
    return lower


def resolve(lower):
    """(keep, kept_by, rounds) of the lists: strand after strand, a strand stays unless a strand before it that stayed pairs with it."""
    keep, kept_by, rounds = [], [], []
    for i, mine in enumerate(lower):
        stayed = [j for j in mine if keep[j]]
        keep.append(0 if stayed else 1)
        kept_by.append(min(stayed) if stayed else i)
        rounds.append(1 + max(rounds[j] for j in mine) if mine else 0)
    return keep, kept_by, rounds


def dedupe(points, offsets, tol):
    """(keep uint8 [N], kept_by int64 [N], rounds int32 [N], lower_offsets int64 [N + 1], lower int32 [n_pairs]) of the contract."""
    lower = lower_lists(points, offsets, tol)
    keep, kept_by, rounds = resolve(lower)
    starts = [0]
    for mine in lower:
        starts.append(starts[-1] + len(mine))
    return (np.array(keep, np.uint8), np.array(kept_by, np.int64), np.array(rounds, np.int32), np.array(starts, np.int64),
            np.array([j for mine in lower for j in mine], np.int32))


def cut(ref, N):
    """The result for the first N strands: a strand's lists, and so its fate, involve the strands before it only."""
    keep, kept_by, rounds, starts, lower = ref
    return keep[:N], kept_by[:N], rounds[:N], starts[:N + 1], lower[:starts[N]]


def pair(points, offsets, tol, i, j):
    """pair(i, j) of the contract, for the checks of the consequences."""
    off = [int(v) for v in offsets]
    tol2 = float(tol) * float(tol)
    for s in range(off[i + 1] - off[i]):
        a, b = [float(v) for v in points[off[i] + s]], [float(v) for v in points[off[j] + s]]
        dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        if not ((dx * dx + dy * dy) + dz * dz <= tol2):
            return False
    return True


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
