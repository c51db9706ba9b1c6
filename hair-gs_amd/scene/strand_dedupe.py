"""Near-copy strands dropped from an exported groom (export_strands.py --dedupe DIST): every other step of the export chain treats a
strand alone, and the chain itself makes strands that are copies of one another.  --interpolate writes the guides and then a strand for
every strand root, and a root that sits on a guide's root gets that guide back; trained models carry duplicated strands of their own
(Stage II merges, Stage III growth), which --points M and --smooth_strands turn into joint-for-joint twins.  A renderer pays for every
copy and shades two coincident transparent curves darker than one, and --select_guides seeds two clusters on one shape.  This is the
chain's first strand-to-strand step: a strand is dropped when an earlier strand that is itself kept has every joint within `tol` of its
own joint of the same index.  Earlier strands win, so trained strands beat interpolated ones (groom.concatenate puts the guides first).

The contract (this module's numpy path, csrc/hgs_dedupe.hip and the loop restatement in tests/dedupe_reference.py state the same
thing).  All arithmetic is float64 on the float32 inputs, with one rounding per operation, in exactly the order written (the kernel
file is built with -ffp-contract=off).

Inputs.  points float32 [N*M, 3].  offsets int64 [N + 1] (strand_collide.check_offsets): every strand has the same number M >= 2 of
points (strand_guides.strand_points raises ValueError for ragged strands, the device wrapper HgsError; the driver says that --points
M > 0 is needed).  tol float64.

Parameter check (check_parameters raises ValueError; the device wrapper raises HgsError; the C entry points return 1).  tol is finite
and >= 0.

Pair.  tol2 = tol*tol, formed once.  For strands i != j, pair(i, j) holds iff d2_s = (dx*dx + dy*dy) + dz*dz <= tol2 for EVERY joint
s = 0 .. M-1, with dx = x_i[s].x - x_j[s].x and so on: all M joints, not a sample.  The relation is symmetric (dx and -dx have one
square).  A strand with a NaN or an infinity pairs with nothing: its d2 at that joint is a NaN or +inf and the comparison is false, so
no rule of its own is needed (the report still counts such strands).  With finite float32 inputs nothing overflows: a difference is
below 2^129, a sum of three squares below 2^260.  The SET of pairs is the contract; how a path finds it -- the order of the joint
tests, an early exit, a test of the root joint in front, chunks -- is its own business, and every path returns exactly that set.

Lower-neighbour lists.  lower_offsets int64 [N + 1], lower int32 [n_pairs]: for every i the j < i with pair(i, j), ascending in j.
n_pairs above MAX_PAIRS = 2^27 (512 MiB of list: a tol that glues the groom together) is refused: ValueError on the numpy path,
HgsError on the device path.  This is a memory limit, not a measurement.

Resolution: the lexicographically first maximal independent set -- "keep a strand unless a kept earlier strand pairs with it", in
ascending index.
    keep[i] = 1 iff no j in lower(i) has keep[j] = 1.
    kept_by[i] = i for a kept strand, else the smallest kept j in lower(i).
    rounds[i] = 0 where lower(i) is empty, else 1 + max(rounds[j] for j in lower(i)).
Both paths compute exactly this in Jacobi rounds over a state per strand (UNDECIDED 0, KEPT 1, DROPPED 2): strands without lower
neighbours start KEPT with round 0; in round r = 1, 2, ... every UNDECIDED strand whose lower neighbours are all decided in the state at
the round's START is decided -- DROPPED where one of them is KEPT, else KEPT -- with rounds = r.  A strand is therefore decided in the
first round at whose start all its lower neighbours are decided, which is the rule above, and the loop ends within N rounds: each
round decides the lowest undecided strand.

Outputs (Dedupe).  keep uint8 [N], kept_by int64 [N], rounds int32 [N], lower_offsets int64 [N + 1], lower int32 [n_pairs].  The
result is the kept strands in order with every bit of their points, attributes, ids and lengths (strand_simplify.take_strands).

Consequences.  No two kept strands pair (the later one would have seen the earlier one kept).  Every dropped strand pairs with its
kept_by, which is kept and earlier.  Running the step on its own output with the same tol drops nothing (no pair is left among the
kept strands, and the pairs do not depend on the other strands).  tol = 0 drops exact copies only (d2 <= 0 means every difference
is 0; -0.0 and 0.0 are one value).  A chain 0 ~ 1 ~ 2 ~ 3 ~ ... with no other pairs keeps 0, 2, 4, ... and takes as many rounds as it
is long (strand c is decided in round c).

Known limits.  Correspondence is by joint index: a short strand that lies along a longer one, or one resampled differently, is not
found.  Priority is the index, not length or quality.  The dropped strands' multiplicity is reported (groups, largest_group) but not
turned into a width or a weight of the strand that stays.  Pairing is not transitive: of a chain, every other strand stays.  Worst-case
rounds equal N (one host read each on the device).  The search is all-pairs -- N (N - 1) / 2 root tests -- on both paths.

device=None: numpy, the root test in blocks of strands against all earlier ones under a fixed element budget (BUDGET), the remaining
joints for the pairs that pass it.  device="cuda": hgs_dedupe_count / hgs_dedupe_fill / hgs_dedupe_resolve on torch tensors; the
offsets are a torch.cumsum of the counts, whose total is the search's one size synchronisation, and the host reads one word per
resolve round, the count of strands still undecided.  The caller chooses; neither falls back to the other."""
import math
from typing import NamedTuple

import numpy as np

from scene.strand_collide import _check_points, check_offsets
from scene.strand_guides import strand_points
from scene.strand_simplify import take_strands

UNDECIDED, KEPT, DROPPED = range(3)
MAX_PAIRS = 1 << 27        # entries of `lower` either path will make (512 MiB of int32)
BUDGET = 1 << 22           # elements of one vectorised block of the numpy path


class Dedupe(NamedTuple):
    keep: np.ndarray           # uint8 [N]: 1 for a strand that stays
    kept_by: np.ndarray        # int64 [N]: the strand itself, or the kept earlier strand that replaces it
    rounds: np.ndarray         # int32 [N]: the Jacobi round that decided the strand
    lower_offsets: np.ndarray  # int64 [N + 1]
    lower: np.ndarray          # int32 [n_pairs]: every strand's lower neighbours, ascending


def check_parameters(tol):
    """tol of the contract as a float, or ValueError."""
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"tol = {tol!r}: a finite distance >= 0") from None
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"tol = {tol}: a finite distance >= 0")
    return tol


def too_many(n_pairs):
    """The refusal of more than MAX_PAIRS pairs, in words both paths and the driver use."""
    return (f"{n_pairs} pairs of strands within tol of each other, above the {MAX_PAIRS} the lists may hold: "
            "the distance glues the groom together; choose a smaller one")


# ---- numpy path ------------------------------------------------------------------------------------------------------------------
def _d2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def pairs_numpy(points, offsets, tol, budget=BUDGET):
    """(lower_offsets int64 [N + 1], lower int32 [n_pairs]) of the contract."""
    points = _check_points(points)
    off = check_offsets(offsets, points.shape[0])
    tol = check_parameters(tol)
    N, M = off.shape[0] - 1, strand_points(off)
    if N == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int32)
    p = points.reshape(N, M, 3)
    root = p[:, 0].astype(np.float64)
    tol2 = tol * tol
    step = max(1, int(budget) // N)
    some = max(1, int(budget) // (3 * M))
    count, lists, total = np.zeros(N, np.int64), [], 0
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, N, step):
            b = min(N, a + step)
            i, j = np.nonzero(_d2(root[a:b, None, :], root[None, :b - 1, :]) <= tol2)       # row by row: by i, then ascending j
            i += a
            sel = j < i
            i, j = i[sel], j[sel]
            ok = np.zeros(i.shape[0], bool)
            for q in range(0, i.shape[0], some):                                            # the other joints of the pairs that passed
                ok[q:q + some] = (_d2(p[i[q:q + some], 1:].astype(np.float64), p[j[q:q + some], 1:].astype(np.float64)) <= tol2).all(axis=1)
            count += np.bincount(i[ok], minlength=N)
            total += int(ok.sum())
            if total > MAX_PAIRS:                                                           # what is held is let go; the count goes on, for the refusal to name
                lists = []
            else:
                lists.append(j[ok].astype(np.int32))
    if total > MAX_PAIRS:
        raise ValueError(too_many(total))
    return np.concatenate([[0], np.cumsum(count)]).astype(np.int64), np.concatenate(lists + [np.zeros(0, np.int32)])


def resolve_round_numpy(lower_offsets, lower, state, kept_by, rounds, r):
    """One Jacobi round of the contract, the statement hgs_dedupe_resolve makes: (the state after it uint8 [N], the strands still
    undecided); kept_by and rounds are written for the strands the round decides."""
    off = np.asarray(lower_offsets, np.int64)
    near = state[lower]
    n_open = np.concatenate([[0], np.cumsum(near == UNDECIDED)])
    n_kept = np.concatenate([[0], np.cumsum(near == KEPT)])
    decide = (state == UNDECIDED) & (n_open[off[1:]] == n_open[off[:-1]])
    drop = decide & (n_kept[off[1:]] > n_kept[off[:-1]])
    stay = decide & ~drop
    first = np.searchsorted(n_kept, n_kept[off[:-1]] + 1) - 1                       # the list's first kept entry: its smallest kept j
    out = state.copy()
    out[drop], out[stay] = DROPPED, KEPT
    kept_by[drop] = lower[first[drop]]
    kept_by[stay] = np.nonzero(stay)[0]
    rounds[decide] = r
    return out, int(np.count_nonzero(out == UNDECIDED))


def resolve_numpy(lower_offsets, lower):
    """(keep uint8 [N], kept_by int64 [N], rounds int32 [N]) of the contract from the lists."""
    off = np.asarray(lower_offsets, np.int64)
    N = off.shape[0] - 1
    state = np.where(off[1:] == off[:-1], KEPT, UNDECIDED).astype(np.uint8)
    kept_by, rounds = np.arange(N, dtype=np.int64), np.zeros(N, np.int32)
    left, r = int(np.count_nonzero(state == UNDECIDED)), 0
    while left:
        r += 1
        state, left = resolve_round_numpy(off, lower, state, kept_by, rounds, r)
    return (state == KEPT).astype(np.uint8), kept_by, rounds


def dedupe_numpy(points, offsets, tol, budget=BUDGET):
    """Dedupe of the contract, by numpy."""
    lower_offsets, lower = pairs_numpy(points, offsets, tol, budget)
    return Dedupe(*resolve_numpy(lower_offsets, lower), lower_offsets, lower)


# ---- device path -----------------------------------------------------------------------------------------------------------------
def _strands_of(rt, points, offsets):
    """(points, N, M) of device tensors points float32 [N*M, 3] and offsets int64 [N + 1], or HgsError (one synchronisation)."""
    import torch
    points = rt.require_gpu_tensor(points, "points", torch.float32)
    offsets = rt.require_gpu_tensor(offsets, "offsets", torch.int64)
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise rt.HgsError(f"dedupe_device: points {tuple(points.shape)} and offsets {tuple(offsets.shape)}; [N*M, 3] and [N + 1] expected")
    N = int(offsets.shape[0]) - 1
    if N == 0:
        return points, 0, 0
    n = offsets[1:] - offsets[:-1]
    M, lo, hi, a, b = (int(v) for v in torch.stack([n[0], n.min(), n.max(), offsets[0], offsets[-1]]).tolist())
    if lo != hi or M < 2 or a != 0 or b != points.shape[0]:
        raise rt.HgsError(f"dedupe_device: strands of {lo} to {hi} points over {b - a} of {points.shape[0]} points: every strand must have "
                          "the same number M >= 2 of points, and the offsets must tile the points")
    return points, N, M


def count_device(points, N, M, tol):
    """hgs_dedupe_count on a device tensor: counts int32 [N, DEDUPE_PARTS] (include/hgs.h: every strand's walk is cut into that many
    parts of ascending j; a row sums to the strand's lower neighbours)."""
    import torch
    import hgs_runtime as rt
    counts = torch.empty((N, rt.DEDUPE_PARTS), dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_dedupe_count(rt.current_stream(), N, M, int(points.shape[0]), rt.ptr(points), tol, rt.ptr(counts)))
    return counts


def fill_device(points, N, M, tol, starts, n_pairs):
    """hgs_dedupe_fill on device tensors: lower int32 [n_pairs]."""
    import torch
    import hgs_runtime as rt
    lower = torch.empty(int(n_pairs), dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_dedupe_fill(rt.current_stream(), N, M, int(points.shape[0]), rt.ptr(points), tol, rt.ptr(starts),
                                          int(n_pairs), rt.ptr(lower)))
    return lower


def pairs_device(points, N, M, tol):
    """(lower_offsets int64 [N + 1], lower int32 [n_pairs]) on the device: count, torch.cumsum, fill; the total is read once."""
    import torch
    import hgs_runtime as rt
    counts = count_device(points, N, M, tol)
    ends = torch.cumsum(counts.view(-1), 0, dtype=torch.int64)                      # the parts ascend in j: flattened, they are the list's order
    n_pairs = int(ends[-1])                                                         # the search's one size synchronisation
    if n_pairs > MAX_PAIRS:
        raise rt.HgsError(f"dedupe_device: {too_many(n_pairs)}")
    lower = fill_device(points, N, M, tol, ends - counts.view(-1), n_pairs)
    lower_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=points.device), ends.view(N, -1)[:, -1]]).contiguous()
    return lower_offsets, lower


def resolve_round_device(lower_offsets, lower, state, state_out, r, kept_by, rounds, undecided):
    """hgs_dedupe_resolve on device tensors: one round from `state` into `state_out`; `undecided` (int32 [1]) is added to."""
    import torch
    import hgs_runtime as rt
    with torch.cuda.device(state.device):
        rt.check(rt.lib().hgs_dedupe_resolve(rt.current_stream(), int(state.shape[0]), rt.ptr(lower_offsets), int(lower.shape[0]), rt.ptr(lower),
                                             rt.ptr(state), rt.ptr(state_out), int(r), rt.ptr(kept_by), rt.ptr(rounds), undecided.data_ptr()))


def resolve_device(lower_offsets, lower):
    """(keep uint8 [N], kept_by int64 [N], rounds int32 [N]) on the device from the lists: Jacobi rounds, one word read per round."""
    import torch
    import hgs_runtime as rt
    N, dev = int(lower_offsets.shape[0]) - 1, lower_offsets.device
    state = (lower_offsets[1:] == lower_offsets[:-1]).to(torch.uint8)               # KEPT where there is no lower neighbour, else UNDECIDED
    other = torch.empty_like(state)
    kept_by, rounds = torch.arange(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    r, words = 0, None
    while lower.shape[0]:
        if r % 64 == 0:
            words = torch.zeros(64, dtype=torch.int32, device=dev)
        word = words[r % 64:r % 64 + 1]
        r += 1
        resolve_round_device(lower_offsets, lower, state, other, r, kept_by, rounds, word)
        state, other = other, state
        if int(word) == 0:                                                          # the round's one synchronisation
            break
        if r > N:
            raise rt.HgsError(f"dedupe_device: {r} rounds for {N} strands: the lists are not lower-neighbour lists")
    return (state == KEPT).to(torch.uint8), kept_by, rounds


def dedupe_device(points, offsets, tol):
    """Dedupe of the contract by the HIP kernels, on device tensors points float32 [N*M, 3] and offsets int64 [N + 1]; the result's
    tensors stay on the device."""
    import torch
    import hgs_runtime as rt
    points, N, M = _strands_of(rt, points, offsets)
    try:
        tol = check_parameters(tol)
    except ValueError as e:
        raise rt.HgsError(f"dedupe_device: {e}") from None
    dev = points.device
    if N == 0:
        empty = lambda dtype, n=0: torch.zeros(n, dtype=dtype, device=dev)
        return Dedupe(empty(torch.uint8), empty(torch.int64), empty(torch.int32), empty(torch.int64, 1), empty(torch.int32))
    lower_offsets, lower = pairs_device(points, N, M, tol)
    return Dedupe(*resolve_device(lower_offsets, lower), lower_offsets, lower)


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def report_of(points, offsets, res):
    """The report of dedupe_strands from the host arrays of either path: one set of numpy statements for both."""
    off = np.asarray(offsets, np.int64)
    N = off.shape[0] - 1
    M = int(off[1] - off[0]) if N else 0
    kept = res.keep != 0
    bad = ~np.isfinite(points.reshape(N, -1)).all(axis=1) if N else np.zeros(0, bool)
    followers = np.bincount(res.kept_by[~kept], minlength=N) if N else np.zeros(0, np.int64)
    return dict(strands=int(N), kept=int(kept.sum()), dropped=int(N - kept.sum()), nonfinite=int(bad.sum()), pairs=int(res.lower.shape[0]),
                rounds=int(res.rounds.max()) if N else 0, groups=int(np.count_nonzero(followers)),
                largest_group=int(followers.max()) if N else 0, joints_before=int(N * M), joints_after=int(kept.sum()) * M)


def dedupe_strands(strands, tol, device=None):
    """`strands` (a StrandExport of strands with the same number of points) without its near copies, see the module docstring:
    (StrandExport, report).  report: "strands", "kept", "dropped", "nonfinite" (strands with a coordinate that is not finite: they stay),
    "pairs" (the lower-neighbour lists' entries), "rounds" (the most a strand took), "groups" (kept strands that replace at least one
    dropped strand), "largest_group" (the most one replaces), "joints_before", "joints_after".  device=None: numpy; "cuda": the HIP
    kernels."""
    points = _check_points(strands.points)
    off = check_offsets(strands.offsets, points.shape[0])
    tol = check_parameters(tol)
    strand_points(off)
    if device is None:
        res = dedupe_numpy(points, off, tol)
    else:
        if not str(device).startswith("cuda"):
            raise ValueError(f"device = {device!r}: None (numpy) or 'cuda' (the HIP kernels)")
        import torch
        res = Dedupe(*(t.cpu().numpy() for t in dedupe_device(torch.as_tensor(points, device=device), torch.as_tensor(off, device=device), tol)))
    return take_strands(strands, np.nonzero(res.keep)[0]), report_of(points, off, res)
