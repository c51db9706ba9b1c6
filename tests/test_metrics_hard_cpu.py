"""The hard clouds of tests/metrics_cases.py meet the conditions they were built for, and the brute-force statements of
tests/metrics_reference.py agree with the CPU path of loss/metrics.py on them, bit for bit, with no point left out.
`pytest -s` prints each case's figures."""
import numpy as np
import pytest

from tests import metrics_cases as MC
from tests import metrics_reference as R

NAMES = MC.case_names()
CPU_NAMES = [n for n in NAMES if MC.get(n).cpu_comparable]
STRAND_NAMES = [n for n in NAMES if MC.get(n).has_strands]


def _live_pairs(c):
    return [k for k in range(c.K) if k not in c.dead_pairs]


@pytest.mark.parametrize("name", NAMES)
def test_every_pair_has_matched_and_unmatched_points_and_pairs_differ(name):
    """An all-zero, all-one or pair-blind kernel fails every case.  Pairs whose cosine is 1.5 or NaN are matched by nothing,
    which is what they are there for; a case of one A point has that point in under one pair and out under another."""
    c = MC.get(name)
    for bidir in c.bidirectional:
        m = MC.expected_masks(name, bidir)
        cnt = R.counts(m, c.K)
        print(f"{name} bidirectional={int(bidir)} nA={len(m)} nB={len(c.b_pts)} matched per pair={cnt}")
        assert all(cnt[k] == 0 for k in c.dead_pairs)
        live = _live_pairs(c)
        if len(m) == 1:
            assert 0 < bin(int(m[0])).count("1") < len(live)
        else:
            assert all(0 < cnt[k] < len(m) for k in live), cnt
        cols = {tuple(((m >> np.uint32(k)) & 1).tolist()) for k in live}
        assert len(cols) >= 2
        if c.K == 32:
            assert 0 < cnt[31] < len(m)


def test_cell_faces_has_points_that_one_ulp_moves_to_another_cell():
    c = MC.get("cell_faces")
    flips = MC.ulp_flips(c)
    print("cell_faces: B points whose cell changes within one ulp:", flips)
    assert flips >= 100 and np.array_equal(c.b_pts[0], c.box[:3])
    h = MC.cell_edge(c.thresholds)
    assert np.array_equal(MC.cells_per_axis(c.box, c.thresholds), [12.0, 12.0, 12.0]) and h == 4e-3 * (1 + 1e-6)
    for name in ("far_from_origin[+1e3]", "far_from_origin[-1e5]"):
        f = MC.get(name)
        assert np.array_equal(f.a_dirs, c.a_dirs) and abs(f.b_pts[0, 0] - c.b_pts[0, 0]) in (1e3, 1e5)


def test_box_rim_points_lie_outside_the_box_at_the_stated_distances():
    c = MC.get("box_rim")
    lo, hi, h = c.box[:3], c.box[3:], MC.cell_edge(c.thresholds)
    rim = c.a_pts[:c.notes["rim_points"]]
    out = np.maximum(np.maximum(lo - rim, rim - hi), 0.0)              # how far outside, per axis
    assert (np.count_nonzero(out, axis=1) >= 1).all()
    assert {1, 2, 3} == set(np.count_nonzero(out, axis=1).tolist())    # faces, edges and the corner
    dist = np.linalg.norm(out, axis=1).reshape(-1, 4)
    print("box_rim: distances outside the box / h:", dist[0] / h, "cells:", MC.cells_per_axis(c.box, c.thresholds))
    assert np.allclose(dist / h, np.array([4e-3 / h, 4e-3 / h, 1.0, 2.5]), rtol=1e-7)
    m = MC.expected_masks("box_rim", False)[:len(rim)].reshape(-1, 4)
    assert (m[:, 0] == 4).all() and (m[:, 1:] == 0).all()             # just under r_max: in under the widest pair; the rest: out
    f = np.floor((rim - lo) / h)
    dims = MC.cells_per_axis(c.box, c.thresholds)
    assert (f == -1).any() and (f == dims).any() and ((f < -1) | (f > dims)).any()
    assert np.allclose(c.extra_boxes[0], np.concatenate([lo - 3.3 * h, hi + 3.3 * h]))


def test_flat_boxes_and_the_cell_limit_have_the_stated_cells():
    want = {"coplanar": (False, False, True), "collinear": (False, True, True), "single": (True, True, True), "coincident": (True, True, True)}
    for k, one in want.items():
        c = MC.get(f"flat_boxes[{k}]")
        dims = MC.cells_per_axis(c.box, c.thresholds)
        print(f"flat_boxes[{k}]: cells per axis", dims)
        assert tuple((dims == 1).tolist()) == one and tuple((c.box[:3] == c.box[3:]).tolist()) == one
    assert len(MC.get("flat_boxes[single]").b_pts) == 1 and len(MC.get("flat_boxes[coincident]").b_pts) == 300
    assert len(np.unique(MC.get("flat_boxes[coincident]").b_strand)) == 5
    c = MC.get("cell_limit")
    assert MC.cells_per_axis(c.box, c.thresholds)[0] == float(MC.MAX_CELLS)
    b = MC.cell_limit_points(1)[2]
    assert MC.cells_per_axis(np.concatenate([b.min(0), b.max(0)]), c.thresholds)[0] == float(MC.MAX_CELLS + 1)


def test_table_sizes_cross_the_doublings_and_buckets_hold_several_cells():
    for n_b in MC.TABLE_NB:
        c = MC.get(f"table_sizes[{n_b}x256]")
        assert len(c.b_pts) == n_b
        cells, occupied, per_bucket = MC.bucket_figures(c)
        print(f"table_sizes nB={n_b}: buckets={MC.table_buckets(n_b)} cells in the box={cells} occupied={occupied} most cells in a bucket={per_bucket}")
        if n_b > 1:
            assert cells > 4 * n_b and occupied > n_b // 2 and per_bucket >= 2
        for n_a in MC.TABLE_NA:
            assert len(MC.get(f"table_sizes[{n_b}x{n_a}]").a_pts) == n_a
    assert [MC.table_buckets(n) for n in (512, 513, 1024, 1025)] == [1024, 2048, 2048, 4096]
    big = MC.get("table_sizes[131073x2000]")
    assert MC.table_buckets(len(big.b_pts)) // MC.SCAN_CHUNK == 512 and len(big.a_pts) == 2000 and big.pruned


def test_the_pruned_reference_equals_brute_force_on_a_slice():
    """The tree only prunes: on 150 A points of the large case, all 131 073 B points tested one by one give the same masks."""
    c = MC.get("table_sizes[131073x2000]")
    want = R.match_masks(c.a_pts[:150], c.a_dirs[:150], c.b_pts, c.b_dirs, c.thresholds, True, chunk=50)
    assert np.array_equal(want, MC.expected_masks(c.name, True)[:150]) and want.any()


def test_dot_edges_has_every_stated_edge_and_exact_dots():
    c = MC.get("dot_edges")
    u, v = c.a_dirs, c.b_dirs
    with np.errstate(invalid="ignore"):
        d1 = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
        d2 = u[:, 0] * v[:, 0] + (u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2])
        d3 = (u[:, 0] * v[:, 0] + u[:, 2] * v[:, 2]) + u[:, 1] * v[:, 1]
        d4 = np.einsum("ij,ij->i", u, v)
    for d in (d2, d3, d4):
        assert np.array_equal(d1, d, equal_nan=True)
    near = np.linalg.norm(c.a_pts - c.b_pts, axis=1) < 2e-3
    m = {bidir: MC.expected_masks("dot_edges", bidir) for bidir in (False, True)}
    below = np.nextafter(0.5, 0.0)
    for dot, bit, want in ((0.5, 0, True), (below, 0, False), (0.0, 1, True), (0.0, 2, True), (-1.0, 3, True), (-1.0, 1, False), (1.0, 4, True)):
        rows = near & (d1 == dot)
        assert rows.any() and (((m[False][rows] >> np.uint32(bit)) & 1) == int(want)).all(), (dot, bit)
    assert (m[True][near & (d1 == -1.0)] == 0b111111).all()              # antiparallel: every pair when bidirectional
    assert (m[False][near & np.isnan(d1)] == 0).all() and (near & np.isnan(d1)).sum() >= 60
    assert (m[False][near & (d1 == np.inf)] == 0b111111).all() and (m[False][near & (d1 == -np.inf)] == 0).all()
    assert (m[True][near & (d1 == -np.inf)] == 0b111111).all()
    zero = near & (np.abs(u).sum(1) == 0) & np.isfinite(v).all(1)
    assert zero.sum() >= 20 and (m[False][zero] & 0b110 == 0b110).all() and np.signbit(d1[zero]).any() and not np.signbit(d1[zero]).all()
    print("dot_edges: couples", len(u), "NaN dots", int(np.isnan(d1).sum()), "infinite dots", int(np.isinf(d1).sum()))


def test_non_finite_points_stand_on_both_sides_and_never_match():
    c = MC.get("non_finite_points")
    bad_a, bad_b = ~np.isfinite(c.a_pts).all(1), ~np.isfinite(c.b_pts).all(1)
    print("non_finite_points: A", int(bad_a.sum()), "B", int(bad_b.sum()), "box", c.box)
    assert bad_a.sum() >= 40 and bad_b.sum() >= 40 and np.isfinite(c.box).all() and not c.cpu_comparable
    for arr in (c.a_pts, c.b_pts):
        assert np.isnan(arr).any() and (arr == np.inf).any() and (arr == -np.inf).any()
    for bidir in (False, True):
        m = MC.expected_masks(c.name, bidir)
        assert (m[bad_a] == 0).all()
        # their neighbours' bits are those of the cloud without the non-finite points
        assert np.array_equal(m[~bad_a], R.match_masks(c.a_pts[~bad_a], c.a_dirs[~bad_a], c.b_pts[~bad_b], c.b_dirs[~bad_b], c.thresholds, bidir))


def test_radii_span_and_all_pairs_have_the_stated_thresholds():
    c = MC.get("radii_span")
    r, cs = c.thresholds[:, 0], c.thresholds[:, 1]
    assert c.K == 6 and r.min() == 1e-4 and r.max() == 1e-2 and list(r) != sorted(r) and len(set(r)) == 5
    assert list(cs[:5]) == [1.0, 0.5, 0.0, -1.0, 1.5] and np.isnan(cs[5]) and c.dead_pairs == (4, 5)
    # the couples at exactly r_k: in under every live pair with r >= r_k, and out one ulp beyond
    n = c.notes["exact_couples"]
    ea, eb = c.a_pts[-n:], c.b_pts[-n:]
    d = eb - ea
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    m = MC.expected_masks("radii_span", False)[-n:]
    for t in range(n):
        k = t // 2
        assert (d2[t] == r[k] * r[k]) == (t % 2 == 0) and d2[t] >= r[k] * r[k]
        assert m[t] == sum(1 << q for q in range(4) if (r[q] > r[k] or (r[q] == r[k] and t % 2 == 0))), (t, bin(m[t]))
    assert (d2 == (r * r).max()).sum() == 1
    assert MC.get("all_pairs").K == 32


def test_vote_cases_have_the_stated_entries():
    for cap in MC.CAPACITIES:
        c = MC.get(f"vote_capacity[{cap}]")
        for bidir in (False, True):
            best, entries = MC.expected_votes(c.name, bidir)
            print(f"{c.name} bidirectional={int(bidir)}: entries {entries.tolist()} best {best.tolist()}")
            assert entries.tolist() == [cap - 1, cap, cap + 1, 0] == c.notes["want_entries"]
            assert best[1].tolist() == [cap // 2, (cap + 1) // 2, (cap + 2) // 2, 0] and (best[0] <= best[1]).all()
    c = MC.get("vote_shapes[mixed]")
    assert np.diff(c.offsets).tolist()[:6] == [1, 2, 9, 10, 256, 1000]
    assert c.b_strand.max() == 100_000 and c.b_strand.min() == 0
    for bidir in (False, True):
        best, entries = MC.expected_votes(c.name, bidir)
        print(f"{c.name} bidirectional={int(bidir)}: entries {entries.tolist()}")
        assert 64 < entries[4] <= 2048 and 1000 <= entries[5] <= 2048 and (entries[:4] <= 64).all()
        s = c.notes["special"]                      # the constructed strand: 5 strands + 1 vote of five points + 1 strand by two points + nothing
        assert entries[s] == 7 and best[:, s].tolist() == [1, 1, 1, 1]
        lo = int(c.offsets[s])
        bits = R.pair_bits(c.a_pts[lo:lo + 4], c.a_dirs[lo:lo + 4], c.b_pts, c.b_dirs, c.thresholds, bidir)
        assert sorted(bits[2][bits[2] != 0].tolist()) == [0b1000, 0b1111] and (bits[3] == 0).all()
        assert np.count_nonzero(bits[0]) == 5 and np.count_nonzero(bits[1]) == 5
    c = MC.get("vote_shapes[S=3000]")
    entries = MC.expected_votes(c.name, True)[1]
    assert len(c.offsets) == 3001 and (entries > 1).sum() > 100 and (entries == 0).sum() > 100
    assert len(MC.get("vote_shapes[S=1]").offsets) == 2
    for order in (0, 1):
        c = MC.get(f"vote_strand_numbers[order{order}]")
        assert (c.b_strand == -1).sum() >= 6 and (c.b_strand == -2 ** 31).sum() >= 6 and c.capacities == (4, 2048)
        best, entries = MC.expected_votes(c.name, True)
        print(f"{c.name}: entries {sorted(set(entries.tolist()))} best max {best.max()}")
        assert best.max() == 2 and (entries == 4).sum() >= 8 and (entries == 16).sum() >= 12
        # the same with ordinary numbers
        b2, e2 = R.strand_votes(c.a_pts, c.a_dirs, c.offsets, c.b_pts, c.b_dirs, MC.renumbered(c.b_strand), c.thresholds, True)
        assert np.array_equal(best, b2) and np.array_equal(entries, e2)
    a, b = MC.get("vote_strand_numbers[order0]"), MC.get("vote_strand_numbers[order1]")
    assert not np.array_equal(a.b_pts, b.b_pts) and np.array_equal(np.sort(a.b_pts, 0), np.sort(b.b_pts, 0))


# ---- against the CPU path --------------------------------------------------------------------------------------------------
def _margin_ok(c, bidir):
    """No candidate within the largest radius has a dot within 1e-12 of a cos_k, unless that dot is the same in every
    summation order (then it may equal cos_k exactly)."""
    bits_r = np.array([[c.thresholds[:, 0].max() * (1 + 1e-9), -np.inf]])
    worst = np.inf
    for i0 in range(0, len(c.a_pts), 512):
        s = slice(i0, i0 + 512)
        if c.pruned:
            from scipy.spatial import cKDTree
            lists = cKDTree(c.b_pts).query_ball_point(c.a_pts[s], bits_r[0, 0])
            i = np.repeat(np.arange(len(lists)), [len(x) for x in lists])
            j = np.array([t for x in lists for t in x], np.int64)
        else:
            i, j = np.nonzero(R.pair_bits(c.a_pts[s], c.a_dirs[s], c.b_pts, c.b_dirs, bits_r, False))   # (a NaN dot never matches: no margin needed)
        u, v = c.a_dirs[s][i], c.b_dirs[j]
        with np.errstate(invalid="ignore"):
            d1 = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
            d2 = u[:, 0] * v[:, 0] + (u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2])
            d3 = np.einsum("ij,ij->i", u, v)
        fragile = ~((d1 == d2) & (d1 == d3)) & np.isfinite(d1)
        d = np.abs(d1[fragile]) if bidir else d1[fragile]
        for cs in c.thresholds[:, 1]:
            if np.isfinite(cs) and d.size:
                worst = min(worst, float(np.abs(d - cs).min()))
    return worst


@pytest.mark.parametrize("name", CPU_NAMES)
def test_brute_force_equals_the_cpu_path_bit_for_bit(name):
    from loss.metrics import HairEvalData, _csr_matches
    c = MC.get(name)
    A, B = HairEvalData(c.a_pts, c.a_dirs), HairEvalData(c.b_pts, c.b_dirs)
    for bidir in c.bidirectional:
        margin = _margin_ok(c, bidir)
        print(f"{name} bidirectional={int(bidir)}: smallest |dot - cos_k| over order-dependent dots = {margin:.3g}")
        assert margin >= 1e-12
        got = np.zeros(len(c.a_pts), np.uint32)
        for k, (r, cs) in enumerate(c.thresholds):
            rows, _ = _csr_matches(A, B, r, cs, bidir)
            got[np.unique(rows)] |= np.uint32(1 << k)
        want = MC.expected_masks(name, bidir)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, bidir, "points that differ:", bad.size, "first:", int(bad[0]), bin(want[bad[0]]), bin(got[bad[0]]))


@pytest.mark.parametrize("name", [n for n in STRAND_NAMES if n in CPU_NAMES and MC.get(n).angles is not None])
def test_votes_and_metrics_equal_pct_matched_points(name):
    """strand_votes / metrics_from_counts against pct_matched_points (recall direction with strand consistency, precision
    direction without), the floats bit for bit."""
    from loss.metrics import HairEvalData, pct_matched_points
    c = MC.get(name)
    gt = HairEvalData(c.a_pts, c.a_dirs, c.a_strand)
    pred = HairEvalData(c.b_pts, c.b_dirs, c.b_strand.astype(np.int64))
    sizes = np.diff(c.offsets)
    keep = sizes > 0                                                    # (np.unique does not see a strand without points)
    for bidir in c.bidirectional:
        best, _ = MC.expected_votes(name, bidir)
        rc = R.counts(MC.expected_masks(name, bidir), c.K)
        pc = R.counts(MC.expected_reverse_masks(name, bidir), c.K)
        want = R.metrics_from_counts(pc, len(c.b_pts), rc, len(c.a_pts), best[:, keep], sizes[keep], bidir)
        sfx = "(b)" if bidir else ""
        for k, (r, ang) in enumerate(zip(c.thresholds[:, 0], c.angles)):
            recall, cons = pct_matched_points(gt, pred, r, ang, bidir, True)
            precision, _ = pct_matched_points(pred, gt, r, ang, bidir, False)
            for nm, v in (("recall", recall), ("precision", precision), ("strand_consistency", cons)):
                assert np.float64(v).tobytes() == np.float64(want[nm + sfx][k]).tobytes(), (name, bidir, k, nm, v, want[nm + sfx][k])


def test_all_pairs_takes_two_passes_through_compute_metrics():
    from loss.metrics import HairEvalData, compute_metrics
    c = MC.get("all_pairs")
    gt, pred = HairEvalData(c.a_pts, c.a_dirs, c.a_strand), HairEvalData(c.b_pts, c.b_dirs, c.b_strand)
    radii, angles = list(MC.ALL_RADII) + [2e-3], list(MC.ALL_ANGLES) + [45.0]
    want = R.reference_metrics(pred, gt, radii, angles, True)
    got, _ = compute_metrics(pred, gt, dist_ths=radii, angle_ths=angles, bidirectional=True)
    assert got.keys() == want.keys()
    for k in got:
        assert len(got[k]) == 33 and got[k].tobytes() == np.asarray(want[k], got[k].dtype).tobytes(), k


def test_brute_force_equals_a_plain_loop_on_twenty_points():
    rng = np.random.default_rng(20)
    a, ad, b, bd = MC._cloud(rng, 20, 20, 0.008)
    thr = MC.pairs_of(MC.R3, MC.ANGLES3)
    off, bs = np.array([0, 7, 7, 20]), rng.integers(-3, 3, 20)
    for bidir in (False, True):
        hit = np.zeros((20, 20), np.uint32)
        for i in range(20):
            for j in range(20):
                dx, dy, dz = (float(b[j, t]) - float(a[i, t]) for t in range(3))
                dot = (float(ad[i, 0]) * float(bd[j, 0]) + float(ad[i, 1]) * float(bd[j, 1])) + float(ad[i, 2]) * float(bd[j, 2])
                for k, (r, cs) in enumerate(thr):
                    if (dx * dx + dy * dy) + dz * dz <= r * r and (abs(dot) if bidir else dot) >= cs:
                        hit[i, j] |= 1 << k
        assert np.array_equal(R.pair_bits(a, ad, b, bd, thr, bidir), hit) and 0 < np.count_nonzero(hit) < 400
        assert np.array_equal(R.match_masks(a, ad, b, bd, thr, bidir, chunk=7), np.bitwise_or.reduce(hit, axis=1))
        assert np.array_equal(R.match_masks(a, ad, b, bd, thr, bidir, pruned=True), np.bitwise_or.reduce(hit, axis=1))
        best, entries = R.strand_votes(a, ad, off, b, bd, bs, thr, bidir)
        for s in range(3):
            votes = {(i, int(bs[j]), k) for i in range(off[s], off[s + 1]) for j in range(20) for k in range(3) if hit[i, j] >> k & 1}
            assert entries[s] == len({(i, t) for i, t, _ in votes})
            for k in range(3):
                per = {}
                for i, t, kk in votes:
                    if kk == k:
                        per[t] = per.get(t, 0) + 1
                assert best[k, s] == max(per.values(), default=0)
        assert entries.sum() > 0
