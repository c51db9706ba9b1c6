"""Hard inputs of the magnet term (loss/losses.py strand_joints_magnet_loss; include/hgs.h hgs_magnet_*): strand polylines
[S, V, 3] float32 that HairGaussianModel.from_strands turns into a model.  Shared by tests/test_magnet_f64_cpu.py and
tests/test_magnet_gpu.py; every case but "big_clustered" is small enough for the loop reference (tests/magnet_reference.py).

from_strands numbers the endpoints strand by strand: strand k of V vertices owns ids k V .. k V + V - 1, its ends are k V and
k V + V - 1.  With V = 2 (one-segment strands) every endpoint is an end, so the position of an end in the list of ends IS its
global id and quirk (c) -- the second neighbour is compared with the partner's GLOBAL id -- really excludes the partner; with
V > 2 the two differ and the comparison hits unrelated ends."""
import numpy as np


def _rng(seed):
    return np.random.default_rng(seed)


def _short_strands(S, V, seed, box=1.0, step=0.02):
    """S strands of V vertices: random starts in a box, short random steps (so that an end's segment partner is close)."""
    r = _rng(seed)
    p = [r.uniform(0, box, size=(S, 3))]
    for _ in range(V - 1):
        d = r.normal(size=(S, 3))
        p.append(p[-1] + step * d / np.linalg.norm(d, axis=1, keepdims=True))
    return np.stack(p, 1).astype(np.float32)


def _collapse(pts, strand, last):
    """The end segment of `strand` (its first one, or its last) collapsed to a point."""
    pts = pts.copy()
    if last:
        pts[strand, -2] = pts[strand, -1]
    else:
        pts[strand, 1] = pts[strand, 0]
    return pts


def _multi():
    from synthetic import strand_polylines
    return strand_polylines(300, 12, seed=4) * 30.0          # ends 0, 12, 13, 25, ...


def _duplicates():
    pts = _short_strands(40, 4, 11)
    pts[5, 0] = pts[2, 0]            # exact duplicates of ends: zero distances, the smaller position first
    pts[9, -1] = pts[2, 0]
    pts[17, 0] = pts[30, -1]
    return pts


def _coincident():
    pts = _short_strands(12, 3, 12)
    pts[:, 0] = 0.25
    pts[:, -1] = 0.25                # every end at one point: all distances 0, positions decide everything
    return pts


def _lattice():
    """Ends on a lattice with power-of-two coordinates: distances are exact in float32 and float64, the ties are real."""
    pts = np.zeros((25, 3, 3), dtype=np.float32)
    for k in range(25):
        i, j = divmod(k, 5)
        pts[k, 0] = (0.5 * i, 0.5 * j, 0.0)
        pts[k, 1] = (0.5 * i + 0.125, 0.5 * j + 0.0625, 0.25)
        pts[k, 2] = (0.5 * i, 0.5 * j, 0.5)
    return pts


def _valid_count(count, seed):
    """Three-vertex strands with exactly `count` valid ends (an odd count: one end segment collapsed)."""
    S = (count + 1) // 2
    pts = _short_strands(S, 3, seed, box=0.5)
    if count % 2:
        pts = _collapse(pts, S // 2, last=False)
    return pts


def _nonfinite():
    pts = _short_strands(30, 4, 13)
    pts[3, 0, 0] = np.nan            # an end with a NaN coordinate: its own segment is not "longer than min_val"
    pts[20, -1, 1] = np.inf          # an end with an infinite one: it stays in the list and compares closer to nothing
    return pts


def _clusters():
    """Two tight clusters far apart: nearly all grid cells are empty, the first radius of a lone end is large."""
    pts = _short_strands(40, 3, 14, box=0.01, step=0.004)
    pts[20:] += np.float32(100.0)
    pts[39] += np.float32(7.0)       # a lone strand beside the second cluster
    return pts


def _line():
    """Every end on one line: a degenerate bounding box (two axes have no extent)."""
    r = _rng(15)
    S = 24
    pts = np.zeros((S, 3, 3), dtype=np.float32)
    x = np.sort(r.uniform(0, 4, size=2 * S)).astype(np.float32)
    pts[:, 0, 0], pts[:, 2, 0] = x[0::2], x[1::2]
    pts[:, 1, 0] = 0.5 * (x[0::2] + x[1::2])
    pts[:, 1, 1] = 0.125             # (the middle vertices leave the line, the ends do not)
    return pts


def _short_lookup():
    """Quirk (d): the selected POSITION is read as a global id; here the endpoints 1 and 2 (middle vertices of strand 0, which
    positions 1 and 2 of the list of ends point at) sit closer than min_val to what the zero-initialised table maps them to --
    endpoint 0 -- so that rows selecting position 1 or 2 fail the neighbour's direction test."""
    pts = _short_strands(10, 4, 16, box=0.05, step=0.01)
    pts[0, 1] = pts[0, 0]
    pts[0, 2] = pts[0, 0]
    # (strand 0's first end segment is collapsed by this: its first end leaves the list, positions shift by one)
    return pts


def _partner_id_hit():
    """Quirk (c) on multi-segment strands: short three-vertex strands far from each other, so that the second neighbour of an
    end is the other end of its own strand.  For the first end of strand 0 that is position 1 -- which equals the GLOBAL id of
    its segment partner, endpoint 1 -- and the statement takes the third neighbour instead; for every other end the comparison
    hits nothing."""
    return _short_strands(12, 3, 17, box=4.0, step=0.01)


def cases():
    """name -> [S, V, 3] float32, in a fixed order."""
    base = _short_strands(30, 5, 7)
    return {
        "no_strands": np.zeros((0, 2, 3), dtype=np.float32),                       # 0 ends
        "one_strand": _short_strands(1, 2, 1),                                     # 2 ends
        "two_strands": _short_strands(2, 2, 2),                                    # 4 ends
        "two_strands_one_collapsed": _collapse(_short_strands(2, 3, 3), 0, False), # 3 valid ends of 4
        "one_segment_3": _short_strands(3, 2, 4),                                  # ends [0..5]: ids == positions
        "one_segment_40": _short_strands(40, 2, 5, box=0.2),
        "multi_segment": _multi(),
        "collapsed_first": _collapse(base, 0, False),
        "collapsed_last": _collapse(base, 29, True),
        "collapsed_middle": _collapse(_collapse(base, 14, True), 15, False),
        "duplicates": _duplicates(),
        "coincident": _coincident(),
        "lattice": _lattice(),
        "valid_255": _valid_count(255, 21),
        "valid_256": _valid_count(256, 22),
        "valid_257": _valid_count(257, 23),
        "nonfinite": _nonfinite(),
        "two_clusters": _clusters(),
        "line": _line(),
        "short_lookup": _short_lookup(),
        "partner_id_hit": _partner_id_hit(),
    }


NAMES = list(cases())


# where the grid path's level changes (csrc/hgs_cellgrid.h cellgrid_level: L = 1 below 1024 ends, 2 below 8192, then 3), one
# below each, on two families of tests/knn_cases.py
LEVEL_EDGE_SIZES = (1023, 1024, 8191, 8192)
LEVEL_EDGE_FAMILIES = ("octants", "clusters")


def level_edge(family, n):
    """[S, 3, 3], S = ceil(n / 2): the points of the knn_cases family as strand ends -- strand k runs from point 2 k through a
    middle vertex 0.02 from it to point 2 k + 1, so every end segment is far longer than min_val and every end is valid.  A set
    of chains has an even number of ends: for an odd n tests/magnet_reference.level_edge_model takes the last end out."""
    from tests import knn_cases as KC
    S = (n + 1) // 2
    ends = KC.large(family, 2 * S).reshape(S, 2, 3)
    d = _rng(31).normal(size=(S, 3))
    mid = ends[:, 0] + 0.02 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.stack([ends[:, 0], mid, ends[:, 1]], 1).astype(np.float32)


def big_clustered():
    """20 000 ends clustered like strand_polylines(10000, 1): the grid path at a size where it is the automatic choice."""
    from synthetic import strand_polylines
    return strand_polylines(10000, 1, seed=9)
