"""Hard clouds for the strand-metric kernels (csrc/hgs_metrics.hip): points on cell faces of the hashed grid, at the rim of
B's box, in boxes with one cell on an axis, at the limit of 2^21 cells, non-finite points and directions, every size at which
the bucket table or the scan takes another path, vote tables filled exactly, and strand numbers that look like the empty marker.
Every case comes from a seed; tests/metrics_reference.py gives the expected integers."""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

R3 = (1e-3, 2.5e-3, 4e-3)                  # the radii of most cases; the cell edge is 4e-3 (1 + 1e-6)
ANGLES3 = (20.0, 35.0, 60.0)
MAX_CELLS = 1 << 21
SCAN_CHUNK = 1024


def cell_edge(thresholds):
    return float(np.asarray(thresholds, np.float64).reshape(-1, 2)[:, 0].max()) * (1.0 + 1e-6)


def pairs_of(radii, angles):
    """thresholds[K][2] = (r_k, cos_k) with the cosine of compute_metrics' angle in degrees."""
    return np.stack([np.asarray(radii, np.float64), np.cos(np.deg2rad(np.asarray(angles, np.float64)))], 1)


@dataclass
class Case:
    name: str
    a_pts: np.ndarray
    a_dirs: np.ndarray
    b_pts: np.ndarray
    b_dirs: np.ndarray
    thresholds: np.ndarray                       # [K][2] (r_k, cos_k)
    offsets: Optional[np.ndarray] = None         # A's strands: runs of its points (A is in strand order)
    b_strand: Optional[np.ndarray] = None        # a strand number per B point
    angles: Optional[tuple] = None               # where the cosines are cos(deg2rad(angles)): the case can go through compute_metrics
    cpu_comparable: bool = True                  # the cKDTree path of loss/metrics.py takes this input
    capacities: tuple = (2048,)                  # vote table sizes to run with
    dead_pairs: tuple = ()                       # pairs whose cosine no dot can reach (1.5, NaN): never matched, by design
    extra_boxes: tuple = ()                      # looser boxes that must give the same result
    pruned: bool = False                         # reference from tree-pruned candidates (the one large case)
    bidirectional: tuple = (False, True)
    reversible: bool = True                      # B against A (compute_metrics' precision pass) is within the cell limit too
    notes: dict = field(default_factory=dict)

    @property
    def K(self):
        return len(self.thresholds)

    @property
    def box(self):
        from loss.metrics import _box
        return _box(np.asarray(self.b_pts, np.float64).reshape(-1, 3)) if len(self.b_pts) else np.zeros(6)

    @property
    def has_strands(self):
        return self.offsets is not None and self.b_strand is not None

    @property
    def a_strand(self):
        return np.repeat(np.arange(len(self.offsets) - 1), np.diff(self.offsets))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _tilted(rng, dirs, sigma=0.45):
    """Directions at a spread of angles (0 .. ~60 degrees) from `dirs`."""
    v = dirs + sigma * rng.normal(size=dirs.shape) * rng.uniform(0, 1, (len(dirs), 1))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _around(rng, b_pts, b_dirs, n, radii, rel=1e-6):
    """n points at r (1 +- rel) from a random B point in a random direction, r drawn from radii; directions tilted from
    that B point's."""
    j = rng.integers(0, len(b_pts), n)
    r = np.asarray(radii)[rng.integers(0, len(radii), n)] * (1.0 + rel * rng.choice([-1.0, 1.0], n))
    return b_pts[j] + r[:, None] * _unit(rng, n), _tilted(rng, b_dirs[j])


def _cloud(rng, n_b, n_a, side, radii=R3):
    """A generic cloud: B uniform in a cube, A around B at assorted distances plus uniform points."""
    b = rng.uniform(0, side, (n_b, 3))
    bd = _unit(rng, n_b)
    n_near = max(n_a - n_a // 3, 1)
    j = rng.integers(0, n_b, n_near)
    a = b[j] + _unit(rng, n_near) * (rng.uniform(0, 1.3, (n_near, 1)) * max(radii))
    ad = _tilted(rng, bd[j])
    a = np.concatenate([a, rng.uniform(-0.1 * side, 1.1 * side, (n_a - n_near, 3))])[:n_a]
    ad = np.concatenate([ad, _unit(rng, n_a - n_near)])[:n_a]
    return a, ad, b, bd


def _strands_by_runs(rng, n, mean_len):
    """offsets of runs of about mean_len points that cover n points."""
    cuts = np.sort(rng.choice(np.arange(1, n), max(n // mean_len - 1, 0), replace=False)) if n > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts, [n]]).astype(np.int64)


# ---- cell faces ------------------------------------------------------------------------------------------------------------
def _cell_faces(seed=0, shift=0.0, name="cell_faces"):
    rng = np.random.default_rng(seed)
    thr = pairs_of(R3, ANGLES3)
    h = cell_edge(thr)
    lo = np.array([0.1037, -0.2011, 0.3119])
    n_b = 600
    m = rng.integers(0, 12, (n_b, 3))
    m[0] = 0
    b = lo + m * h
    nudge = rng.integers(-4, 5, (n_b, 3))
    nudge = np.where(m == 0, np.abs(nudge), nudge)          # (nothing goes below lo: B[0] = lo stays the box's corner)
    nudge[0] = 0
    for _ in range(4):
        b = np.where(nudge > 0, np.nextafter(b, np.inf), np.where(nudge < 0, np.nextafter(b, -np.inf), b))
        nudge = nudge - np.sign(nudge)
    bd = _unit(rng, n_b)
    a, ad = _around(rng, b, bd, 600, R3)
    far = rng.uniform(0, 12 * h, (40, 3)) + lo                # (uniform points: some of them matched by nothing)
    a, ad = np.concatenate([a, far]), np.concatenate([ad, _unit(rng, 40)])
    if shift:
        a, b = a + shift, b + shift                           # translate first: the reference sees the translated values
    off = _strands_by_runs(rng, len(a), 12)
    return Case(name, a, ad, b, bd, thr, offsets=off, b_strand=rng.integers(0, 60, n_b).astype(np.int32), angles=ANGLES3)


def ulp_flips(case):
    """B points whose cell floor((x - lo) / h) on some axis changes when that coordinate moves one ulp."""
    b, lo, h = case.b_pts, case.box[:3], cell_edge(case.thresholds)
    c = np.floor((b - lo) / h)
    up, dn = np.floor((np.nextafter(b, np.inf) - lo) / h), np.floor((np.nextafter(b, -np.inf) - lo) / h)
    return int(((up != c) | (dn != c)).any(1).sum())


# ---- the rim of B's box ----------------------------------------------------------------------------------------------------
def _box_rim(seed=1):
    rng = np.random.default_rng(seed)
    thr = pairs_of(R3, ANGLES3)
    rmax, h = max(R3), cell_edge(thr)
    lo, hi = np.array([0.05, 0.07, -0.03]), np.array([0.05, 0.07, -0.03]) + np.array([5.0, 6.0, 4.0]) * h + 1e-4
    mid = 0.5 * (lo + hi)
    b = [rng.uniform(lo, hi, (150, 3)), lo[None], hi[None]]
    a, anchors = [], []
    dists = (rmax * (1 - 1e-9), rmax * (1 + 1e-9), h, 2.5 * h)
    # outward normals: the six faces, three edges and a corner
    normals = [s * np.eye(3)[ax] for ax in range(3) for s in (-1.0, 1.0)]
    normals += [np.array([-1.0, -1.0, 0.0]), np.array([1.0, 0.0, 1.0]), np.array([0.0, -1.0, 1.0]), np.array([1.0, 1.0, 1.0])]
    for nrm in normals:
        on = np.where(nrm < 0, lo, np.where(nrm > 0, hi, mid))       # a B point on that face / edge / corner
        anchors.append(on)
        for d in dists:
            a.append(on + d * nrm / np.linalg.norm(nrm))
    b.append(np.array(anchors))
    b = np.concatenate(b)
    bd = np.tile([0.0, 0.0, 1.0], (len(b), 1))
    bd[:150] = _unit(rng, 150)
    a = np.array(a)
    ad = np.tile([0.0, 0.0, 1.0], (len(a), 1))
    a2, ad2 = _around(rng, b[:150], bd[:150], 200, R3, rel=0.05)
    a, ad = np.concatenate([a, a2]), np.concatenate([ad, ad2])
    box = np.concatenate([b.min(0), b.max(0)])
    loose = np.concatenate([box[:3] - 3.3 * h, box[3:] + 3.3 * h])
    off = _strands_by_runs(rng, len(a), 8)
    return Case("box_rim", a, ad, b, bd, thr, offsets=off, b_strand=rng.integers(0, 30, len(b)).astype(np.int32), angles=ANGLES3,
                extra_boxes=(loose,), notes={"rim_points": len(normals) * len(dists)})


# ---- boxes with one cell on an axis ----------------------------------------------------------------------------------------
def _flat_boxes(seed=2):
    out = []
    thr = pairs_of(R3, ANGLES3)
    for name in ("coplanar", "collinear", "single", "coincident"):
        rng = np.random.default_rng([seed, len(out)])
        if name == "coplanar":
            b = rng.uniform(0, 0.04, (300, 3)); b[:, 2] = 0.0125
        elif name == "collinear":
            b = rng.uniform(0, 0.08, (300, 3)); b[:, 1:] = (0.25, -0.5)
        elif name == "single":
            b = np.array([[0.3, 0.1, -0.2]])
        else:
            b = np.tile([[0.011, 0.022, 0.033]], (300, 1))
        bd = _unit(rng, len(b))
        a = b[rng.integers(0, len(b), 300)] + _unit(rng, 300) * rng.uniform(0, 1.5, (300, 1)) * max(R3)
        ad = _tilted(rng, bd[rng.integers(0, len(b), 300)], 0.8)
        out.append(Case(f"flat_boxes[{name}]", a, ad, b, bd, thr, offsets=_strands_by_runs(rng, 300, 10),
                        b_strand=(np.arange(len(b)) % 5).astype(np.int32), angles=ANGLES3))
    return out


# ---- the limit of cells per axis -------------------------------------------------------------------------------------------
def cell_limit_points(extra_cells=0):
    """Two B points whose box needs exactly 2^21 (+ extra_cells) cells on x, A points near each; (a, ad, b, bd, thresholds)."""
    rng = np.random.default_rng(3)
    thr = pairs_of(R3, ANGLES3)
    h = cell_edge(thr)
    lo = np.array([0.5, 0.25, -0.125])
    b = np.stack([lo, lo + np.array([(MAX_CELLS - 1 + extra_cells + 0.5) * h, 0.0, 0.0])])
    bd = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    a = np.concatenate([b[j] + _unit(rng, 12) * rng.uniform(0, 1.6, (12, 1)) * max(R3) for j in (0, 1)])
    ad = np.concatenate([_tilted(rng, np.tile(bd[j], (12, 1)), 0.8) for j in (0, 1)])
    return a, ad, b, bd, thr


def cells_per_axis(box, thresholds):
    h = cell_edge(thresholds)
    return np.floor((np.asarray(box[3:]) - np.asarray(box[:3])) / h) + 1.0


def _cell_limit():
    a, ad, b, bd, thr = cell_limit_points(0)
    return Case("cell_limit", a, ad, b, bd, thr, offsets=np.array([0, 12, 24], np.int64), b_strand=np.array([7, 7], np.int32), angles=ANGLES3,
                reversible=False)      # (A's points lie around both ends: their own box needs a cell more than B's, and is refused)


# ---- radii and cosines -----------------------------------------------------------------------------------------------------
def _radii_span(seed=4):
    rng = np.random.default_rng(seed)
    thr = np.array([[3e-3, 1.0], [1e-4, 0.5], [1e-2, 0.0], [1e-3, -1.0], [1e-3, 1.5], [5e-3, np.nan]])
    radii = thr[:, 0]
    n_b = 300
    b = rng.uniform(0, 0.08, (n_b, 3))
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    bd = _unit(rng, n_b)
    bd[:120] = axes[rng.integers(0, 6, 120)]                     # axis directions: dots of exactly 1, 0 and -1
    j = rng.integers(0, n_b, 500)
    r = radii[rng.integers(0, len(radii), 500)] * rng.choice([0.5, 1 - 1e-6, 1 + 1e-6, 1.7], 500)
    a = b[j] + r[:, None] * _unit(rng, 500)
    ad = _tilted(rng, bd[j], 0.9)
    same = (rng.uniform(size=500) < 0.5) & (j < 120)              # an axis direction's own copy: a dot of exactly 1
    ad[same] = bd[j[same]]
    a = np.concatenate([a, rng.uniform(-0.02, 0.1, (40, 3))])
    ad = np.concatenate([ad, axes[rng.integers(0, 6, 40)]])
    # couples on their own, 0.05 apart, at a distance of exactly r_k and one ulp beyond: B at x = 0, A at x = r_k, so that
    # dx = 0 - r_k and d2 = r_k*r_k hold bit for bit (d2 <= r_k*r_k is an equality there; the largest is r2max itself)
    xs = np.array([x for r in radii for x in (r, np.nextafter(r, np.inf))])
    ys = -0.05 * (1 + np.arange(len(xs)))
    eb = np.stack([np.zeros(len(xs)), ys, np.zeros(len(xs))], 1)
    ea = np.stack([xs, ys, np.zeros(len(xs))], 1)
    ex = np.tile([1.0, 0.0, 0.0], (len(xs), 1))
    return Case("radii_span", np.concatenate([a, ea]), np.concatenate([ad, ex]), np.concatenate([b, eb]), np.concatenate([bd, ex]), thr,
                dead_pairs=(4, 5), notes={"exact_couples": len(xs)})


# ---- the direction test ----------------------------------------------------------------------------------------------------
DYADIC_DIRS = np.array([
    [0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [np.nextafter(0.5, 0.0), 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [-0.5, -0.5, 0.0],
    [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.75, 0.25, 0.5], [0.25, -0.75, 0.5], [0.5, 0.0, 0.0], [np.nextafter(0.5, 1.0), 0.0, 0.0],
    [np.nan, 0.0, 0.0], [0.5, np.nan, 0.5], [np.inf, 0.0, 0.0], [-np.inf, 0.5, 0.0], [0.0, 1.0, 0.0], [0.625, 0.625, 0.0]])
DOT_COSINES = (0.5, 0.0, -0.0, -1.0, 1.0, 0.25)


def _dot_edges():
    """Every ordered pair of DYADIC_DIRS as one isolated (A point, B point) couple 1 mm apart, couples 0.05 apart: the mask of
    an A point is its couple's direction test.  Every dot is one product or a sum of exact dyadic products, so it is
    the same in every summation order: (1, 0, 0) . (0.5, 0, 0) = 0.5 equals the cosine and matches, the value one ulp
    below does not.  (The two neighbours of 0.5 stand alone in their vectors, so their dots are one rounded product.)"""
    n = len(DYADIC_DIRS)
    ia, ib = np.divmod(np.arange(n * n), n)
    site = np.stack(np.unravel_index(np.arange(n * n), (7, 7, 7)), 1) * 0.05
    b = site + np.array([0.01, 0.02, 0.03])
    a = b + np.array([0.0, 1e-3, 0.0])
    # two couples out of reach of every radius, so that cos = -1 has an unmatched finite point too
    a[[1, 20]] += 0.01
    thr = np.array([[2e-3, c] for c in DOT_COSINES])
    return Case("dot_edges", a, DYADIC_DIRS[ia], b, DYADIC_DIRS[ib], thr)


# ---- non-finite points -----------------------------------------------------------------------------------------------------
def _non_finite(seed=6):
    rng = np.random.default_rng(seed)
    a, ad, b, bd = _cloud(rng, 400, 400, 0.04)
    bad = (np.nan, np.inf, -np.inf)
    for arr in (a, b):
        rows = rng.choice(len(arr), 45, replace=False)
        for t, i in enumerate(rows):
            if t % 3 == 0:
                arr[i] = bad[(t // 3) % 3]                       # the whole point
            else:
                arr[i, rng.integers(0, 3)] = bad[t % 3]          # one coordinate
    off = _strands_by_runs(rng, len(a), 9)
    return Case("non_finite_points", a, ad, b, bd, pairs_of(R3, ANGLES3), offsets=off, b_strand=rng.integers(0, 40, len(b)).astype(np.int32),
                cpu_comparable=False)


# ---- table sizes -----------------------------------------------------------------------------------------------------------
def table_buckets(n_b):
    t = SCAN_CHUNK
    while t < 2 * n_b:
        t <<= 1
    return t


def cell_bucket(cells, table):
    """The kernel's bucket of integer cells [n][3] (uint64 arithmetic of cell_bucket in csrc/hgs_metrics.hip), for the
    condition that buckets hold several cells."""
    c = np.asarray(cells, np.int64).astype(np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        k = (c[:, 0] << np.uint64(44)) | (c[:, 1] << np.uint64(22)) | c[:, 2]
        k ^= k >> np.uint64(31); k *= np.uint64(0x7FB5D329728EA185); k ^= k >> np.uint64(27)
        k *= np.uint64(0x81DADEF4BC2DD44D); k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)) & np.uint64(table - 1)


def bucket_figures(case):
    """(cells in the box, occupied cells, the most distinct cells in one bucket)."""
    h, box = cell_edge(case.thresholds), case.box
    dims = cells_per_axis(box, case.thresholds)
    cells = np.unique(np.clip(np.floor((case.b_pts - box[:3]) / h), 0, dims - 1).astype(np.int64), axis=0)
    per = np.unique(cell_bucket(cells, table_buckets(len(case.b_pts))), return_counts=True)[1]
    return int(np.prod(dims)), len(cells), int(per.max())


TABLE_NB = (1, 511, 512, 513, 1024, 1025)
TABLE_NA = (1, 255, 256, 257)


def _table_sizes():
    out = []
    for n_b in TABLE_NB:
        for n_a in TABLE_NA:
            rng = np.random.default_rng([7, n_b, n_a])
            side = max(R3) * (2.0 * n_b ** (1 / 3) + 2.0)         # about 8 cells of the box per B point
            a, ad, b, bd = _cloud(rng, n_b, max(n_a, 2), side)
            if n_a == 1:                                          # one point, 2 mm from B[0]: in under the two wider pairs only
                a, ad = b[:1] + np.array([[0.0, 2e-3, 0.0]]), bd[:1].copy()
            out.append(Case(f"table_sizes[{n_b}x{n_a}]", a[:n_a], ad[:n_a], b, bd, pairs_of(R3, ANGLES3)))
    rng = np.random.default_rng([7, 131073])
    a, ad, b, bd = _cloud(rng, 131073, 2000, 0.26)
    out.append(Case("table_sizes[131073x2000]", a, ad, b, bd, pairs_of(R3, ANGLES3), pruned=True))
    return out


# ---- 32 pairs --------------------------------------------------------------------------------------------------------------
ALL_RADII = tuple(np.linspace(1e-3, 6e-3, 32))
ALL_ANGLES = tuple(np.linspace(5, 90, 32))


def _all_pairs(seed=8):
    rng = np.random.default_rng(seed)
    a, ad, b, bd = _cloud(rng, 300, 300, 0.07, ALL_RADII)
    return Case("all_pairs", a, ad, b, bd, pairs_of(ALL_RADII, ALL_ANGLES), offsets=_strands_by_runs(rng, 300, 10),
                b_strand=rng.integers(0, 25, 300).astype(np.int32), angles=ALL_ANGLES)


# ---- votes -----------------------------------------------------------------------------------------------------------------
VOTE_RADII = (2e-3, 3e-3, 4e-3, 4e-3)
VOTE_ANGLES = (20.0, 30.0, 40.0, 90.0)


def _rot_z(v, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([c * v[0] - s * v[1], s * v[0] + c * v[1], v[2]])


def _vote_shapes(seed=9):
    rng = np.random.default_rng(seed)
    thr = pairs_of(VOTE_RADII, VOTE_ANGLES)
    sizes = [1, 2, 9, 10, 256, 1000, 30, 30]
    ap, ad, bp, bd, bs = [], [], [], [], []
    for s, n in enumerate(sizes):
        # strand s runs along x at its own (y, z), 1 mm a step; the last two run 2 mm apart and share B strands
        y, z = (0.02 * s, 0.01) if s < 7 else (0.02 * 6 + 2e-3, 0.01)
        p = np.stack([np.arange(n) * 1e-3, np.full(n, y) + 2e-4 * np.sin(np.arange(n)), np.full(n, z)], 1)
        d = np.tile([1.0, 0.0, 0.0], (n, 1))
        ap.append(p); ad.append(d)
        keep = rng.uniform(size=n) < 0.8 if n > 2 else np.ones(n, bool)
        bp.append(p[keep] + rng.normal(size=(keep.sum(), 3)) * 4e-4)
        bd.append(_tilted(rng, d[keep], 0.7))
        ids = np.where(np.arange(n)[keep] < 0.6 * n, 1000 * s, 1000 * s + 17)      # two B strands per A strand: 0, 17, 1000, ...
        bs.append(np.where(rng.uniform(size=keep.sum()) < 0.03, 99_000 + rng.integers(0, 1000, keep.sum()), ids))
    # the constructed strand, far from the rest (x around 1.5): four points
    base = np.array([1.5, 0.0, 0.0])
    e = np.array([1.0, 0.0, 0.0])
    cp, cd = [], []
    # (a) a point that matches five B strands
    cp.append(base); cd.append(e)
    for t in range(5):
        bp.append((base + 5e-4 * _unit(rng, 1))); bd.append(e[None]); bs.append(np.array([50_000 + t]))
    # (b) five B points of one strand, all matching one point: one vote
    q = base + np.array([0.02, 0.0, 0.0])
    cp.append(q); cd.append(e)
    bp.append(q + 5e-4 * _unit(rng, 5)); bd.append(np.tile(e, (5, 1))); bs.append(np.full(5, 100_000))
    # (c) strand 60000 under pair 0 through one B point (1 mm, 10 degrees) and under pair 3 alone through another (3.5 mm, 80 degrees)
    q = base + np.array([0.04, 0.0, 0.0])
    cp.append(q); cd.append(e)
    bp.append(np.stack([q + [0.0, 1e-3, 0.0], q + [0.0, 0.0, 3.5e-3]])); bd.append(np.stack([_rot_z(e, 10.0), _rot_z(e, 80.0)]))
    bs.append(np.array([60_000, 60_000]))
    # (d) a point that nothing matches
    cp.append(base + np.array([0.06, 0.0, 0.0])); cd.append(e)
    ap.append(np.array(cp)); ad.append(np.array(cd))
    sizes.append(4)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return Case("vote_shapes[mixed]", np.concatenate(ap), np.concatenate(ad), np.concatenate(bp), np.concatenate(bd), thr, offsets=off,
                b_strand=np.concatenate(bs).astype(np.int32), angles=VOTE_ANGLES, capacities=(2048, 64),
                notes={"special": len(sizes) - 1})


def _vote_one_strand(seed=10):
    rng = np.random.default_rng(seed)
    a, ad, b, bd = _cloud(rng, 200, 150, 0.03, VOTE_RADII)
    return Case("vote_shapes[S=1]", a, ad, b, bd, pairs_of(VOTE_RADII, VOTE_ANGLES), offsets=np.array([0, 150], np.int64),
                b_strand=rng.integers(0, 12, 200).astype(np.int32), angles=VOTE_ANGLES, capacities=(2048, 64))


def _vote_many_strands(seed=11):
    rng = np.random.default_rng(seed)
    S = 3000
    sizes = rng.choice([1, 1, 1, 2], S)
    n = int(sizes.sum())
    a = rng.uniform(0, 0.12, (n, 3))
    ad = _unit(rng, n)
    pick = rng.choice(n, 3000, replace=False)
    b = a[pick] + _unit(rng, 3000) * rng.uniform(0, 1.4, (3000, 1)) * 4e-3
    bd = _tilted(rng, ad[pick], 0.8)
    return Case("vote_shapes[S=3000]", a, ad, b, bd, pairs_of(VOTE_RADII, VOTE_ANGLES), offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                b_strand=rng.integers(0, 100_001, 3000).astype(np.int32), angles=VOTE_ANGLES, capacities=(2048, 1))


CAPACITIES = (1, 2, 64, 2048)


def _vote_capacity(cap):
    """Strands of cap - 1, cap and cap + 1 points on a 0.1 lattice, each point with one coincident B point of the strand's
    own two B strands (alternating), so that entries = the point count; and a fourth strand that nothing matches."""
    rng = np.random.default_rng([12, cap])
    sizes = [cap - 1, cap, cap + 1, 3]
    n = sum(sizes)
    side = int(np.ceil(n ** (1 / 3)))
    a = np.stack(np.unravel_index(np.arange(n), (side, side, side)), 1) * 0.1 + np.array([0.013, 0.027, 0.031])
    ad = _unit(rng, n)
    m = n - 3
    b = a[:m].copy()
    bd = ad[:m].copy()
    owner = np.repeat(np.arange(3), sizes[:3])
    local = np.arange(m) - np.concatenate([[0], np.cumsum(sizes)])[owner]
    turn = local % 3 == 1                                         # a third of the B points 45 degrees off: out under pair 0, in under pair 1
    w = _unit(rng, m)
    w -= (w * ad[:m]).sum(1, keepdims=True) * ad[:m]
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    bd[turn] = ((ad[:m] + w) / np.sqrt(2.0))[turn]
    b_strand = (owner * 10 + local % 2).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    thr = pairs_of((1e-3, 1e-3), (20.0, 80.0))
    return Case(f"vote_capacity[{cap}]", a, ad, b, bd, thr, offsets=off, b_strand=b_strand, angles=(20.0, 80.0), capacities=(cap,),
                notes={"want_entries": sizes[:3] + [0]})


def renumbered(b_strand):
    """The same partition of B with ordinary numbers 0 .. n-1."""
    return np.unique(np.asarray(b_strand).astype(np.int64), return_inverse=True)[1].reshape(-1).astype(np.int32)


def _vote_strand_numbers(order):
    """B strands whose numbers are -1 (the bit pattern of an all-ones empty marker) and -2^31 beside ordinary numbers that
    share their home slot in a table of 4 and of 2048 entries (multiplicative hash: a number = -1 mod 2048 starts where -1
    does, a multiple of 2048 where -2^31 does).  Every A strand has two points per B strand of its group, so best = 2 unless
    two strands' counts are added up."""
    rng = np.random.default_rng(13)
    groups = {2048: [[-1, 2047, 4095, 6143, 8191, 10239, 12287, 14335], [-2 ** 31, 0, 2048, 4096, 6144, 2 ** 30, 8192, 5]],
              4: [[-1, 3], [-2 ** 31, 0], [-1, 7], [3, -1]]}
    ap, ad, bp, bd, bs, sizes = [], [], [], [], [], []
    s = 0
    for cap, gs in groups.items():
        for rep in range(6 if cap == 2048 else 2):
            for g in gs:
                ids = list(rng.permutation(g)) if rep else list(g)
                pts = np.stack([np.arange(2 * len(ids)) * 0.05, np.full(2 * len(ids), 0.05 * s), np.zeros(2 * len(ids))], 1)
                d = _unit(rng, len(pts))
                ap.append(pts); ad.append(d)
                bp.append(pts + rng.normal(size=pts.shape) * 2e-4); bd.append(d)
                bs.append(np.repeat(ids, 2))
                sizes.append(len(pts))
                s += 1
    # and one strand that nothing matches
    ap.append(np.array([[0.0, -0.05, 0.0]])); ad.append(_unit(rng, 1)); sizes.append(1)
    a, adir, b, bdir, bstr = np.concatenate(ap), np.concatenate(ad), np.concatenate(bp), np.concatenate(bd), np.concatenate(bs)
    off_dir = rng.uniform(size=len(b)) < 0.25
    bdir[off_dir] = _tilted(rng, bdir[off_dir], 1.5)
    perm = np.arange(len(b)) if order == 0 else np.random.default_rng(14).permutation(len(b))
    return Case(f"vote_strand_numbers[order{order}]", a, adir, b[perm], bdir[perm], pairs_of(VOTE_RADII, VOTE_ANGLES),
                offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), b_strand=bstr[perm].astype(np.int32), angles=VOTE_ANGLES,
                capacities=(4, 2048))


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [_cell_faces(), _box_rim()] + _flat_boxes()
    cases += [_cell_faces(0, 1e3, "far_from_origin[+1e3]"), _cell_faces(0, -1e5, "far_from_origin[-1e5]"), _cell_limit(), _radii_span(),
              _dot_edges(), _non_finite()] + _table_sizes()
    cases += [_all_pairs(), _vote_shapes(), _vote_one_strand(), _vote_many_strands()] + [_vote_capacity(c) for c in CAPACITIES]
    cases += [_vote_strand_numbers(0), _vote_strand_numbers(1)]
    for c in cases:
        for arr in (c.a_pts, c.a_dirs, c.b_pts, c.b_dirs, c.thresholds):
            arr.setflags(write=False)
    return tuple(cases)


def case_names():
    return [c.name for c in all_cases()]


def get(name):
    return next(c for c in all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected_masks(name, bidirectional):
    """match_masks of a case, computed once and shared (read-only)."""
    from tests import metrics_reference as R
    c = get(name)
    m = R.match_masks(c.a_pts, c.a_dirs, c.b_pts, c.b_dirs, c.thresholds, bidirectional, pruned=c.pruned)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected_votes(name, bidirectional):
    """strand_votes of a case with strands, computed once and shared (read-only)."""
    from tests import metrics_reference as R
    c = get(name)
    best, entries = R.strand_votes(c.a_pts, c.a_dirs, c.offsets, c.b_pts, c.b_dirs, c.b_strand, c.thresholds, bidirectional)
    best.setflags(write=False); entries.setflags(write=False)
    return best, entries


@functools.lru_cache(maxsize=None)
def expected_reverse_masks(name, bidirectional):
    """match_masks of B against A (the precision direction of compute_metrics), computed once and shared (read-only)."""
    from tests import metrics_reference as R
    c = get(name)
    m = R.match_masks(c.b_pts, c.b_dirs, c.a_pts, c.a_dirs, c.thresholds, bidirectional)
    m.setflags(write=False)
    return m
