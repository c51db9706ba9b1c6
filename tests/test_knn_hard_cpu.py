"""The references of the neighbour searches against each other on the degenerate clouds of tests/knn_cases.py (no GPU):
the oracle (oracle/knn_oracle.c, the reference's pruned search) against the float32 brute force bit for bit, the float32 brute
forces against float64 within the derived bars (tests/knn_reference.py: 6 u per squared distance, 9 u per mean), what
non-finite points do, the float32 pair statement against the kd-tree's, and the CPU branch of loss.losses.knn3_self."""
import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import knn_cases as KC
from tests import knn_reference as KR

_CACHE = {}


def _small(name):
    if name not in _CACHE:
        p = KC.small(name)
        _CACHE[name] = (p, KR.brute_dist2_f32(p))
    return _CACHE[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", KC.NAMES)
def test_oracle_equals_brute_force_bit_for_bit(name):
    p, brute = _small(name)
    got = O.dist2(p)
    diff = int((_bits(got) != _bits(brute)).sum())
    print(f"KNN_ORACLE {name} P={p.shape[0]} differing words={diff}")
    assert diff == 0


@pytest.mark.parametrize("name", KC.NAMES)
def test_dist2_float32_within_9u_of_float64(name):
    p, b32 = _small(name)
    b64 = KR.brute_dist2_f64(p)
    fin = np.isfinite(b64) & (b64 > 0)
    worst = float((np.abs(b32[fin].astype(np.float64) - b64[fin]) / b64[fin]).max() / KR.U) if fin.any() else 0.0
    print(f"KNN_F64 dist2 {name} worst={worst:.3f} u  zeros={int((b64 == 0).sum())} inf={int(np.isinf(b64).sum())}")
    assert KR.within(b32, b64, 9).all()
    assert np.array_equal(b32 == 0, b64 == 0)
    if name == "lattice_holes":
        # every difference, square and sum is exact in float32: the two precisions differ by the rounding of the division alone
        assert np.array_equal(b32, b64.astype(np.float32))
    if name == "non_finite":
        assert np.isposinf(b32[list(KC.NON_FINITE_ROWS)]).all() and np.isfinite(np.delete(b32, KC.NON_FINITE_ROWS)).all()


@pytest.mark.parametrize("name", KC.NAMES)
def test_knn3_float32_within_6u_of_float64(name):
    p = KC.FAMILIES[name](min(KC.SMALL[name], 3000), 400 + KC.NAMES.index(name))
    d32, i32 = KR.brute_knn3_f32(p)
    d64, i64 = KR.brute_knn3_f64(p)
    fin = np.isfinite(d64) & (d64 > 0)
    worst = float((np.abs(d32[fin].astype(np.float64) - d64[fin]) / d64[fin]).max() / KR.U) if fin.any() else 0.0
    print(f"KNN_F64 knn3 {name} worst={worst:.3f} u")
    assert KR.within(d32, d64, 6).all()
    assert np.array_equal(d32 == 0, d64 == 0)
    assert np.array_equal(i32 < 0, i64 < 0)
    if name == "lattice_holes":
        assert np.array_equal(d32.astype(np.float64), d64) and np.array_equal(i32, i64)


def test_non_finite_points_are_invisible_to_the_others():
    p, _ = _small("non_finite")
    rows = list(KC.NON_FINITE_ROWS)
    full = O.dist2(p)
    keep = np.ones(p.shape[0], bool)
    keep[rows] = False
    assert np.isfinite(p[keep]).all() and not np.isfinite(p[rows]).all(axis=1).any()
    sub = O.dist2(np.ascontiguousarray(p[keep]))
    assert np.array_equal(_bits(full[keep]), _bits(sub))
    assert np.isposinf(full[rows]).all()


def test_margin_cloud_needs_the_margin_of_the_cube_range():
    """What KC.margin_cloud() claims, in the arithmetic of cellgrid_search_kernel / cellgrid_code (csrc/hgs_cellgrid.h): without the
    1.000001 the cube range of point 0 stops one cell short of its third neighbour, and the mean changes."""
    f = np.float32
    p = KC.margin_cloud()
    mn, mx = f(min(0.0, p[:, 0].min())), f(max(0.0, p[:, 0].max()))

    def cell(x):                                   # level 1: two cells per axis
        return int(f(f(f(x) - mn) / f(mx - mn)) * f(1023)) >> 9

    x0, x4 = p[0, 0], p[4, 0]
    a = f(x0 - x4)
    assert float(a) < float(x0) - float(x4)                                    # the difference rounds down
    assert cell(x4) == 0 and cell(np.nextafter(x4, f(1))) == 1 == cell(x0)     # point 4 is the last float of its cell
    d = p - p[0]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2[1] == d2[2] == 0 and d2[4] == f(a * a) and d2[3] == np.nextafter(d2[4], f(1)) and (d2[5:] > 1).all()
    for r2 in (d2[3], d2[4]):                                                  # (whichever of the two the lane holds as its radius)
        r0 = np.sqrt(r2)
        assert r0 == a
        assert cell(f(x0 - r0)) == 1                                           # no margin: the range stops in point 0's own cell
        assert cell(f(x0 - f(r0 * f(1.000001)))) == 0                          # with it: point 4's cell is walked
    ref = KR.brute_dist2_f32(p)
    assert ref[0] == f(d2[4] / f(3)) != f(d2[3] / f(3))                        # missing point 4 changes the result
    assert np.array_equal(_bits(O.dist2(p)), _bits(ref))


@pytest.mark.parametrize("name", KC.PAIR_NAMES)
def test_float32_pair_statement_against_the_kdtree(name):
    pos, dirs, r, min_cos, bidir, on_lattice = KC.pair_cases()[name]
    pairs, dist = KR.brute_pairs_f32(pos, dirs, r, min_cos, bidir)
    got = set(map(tuple, pairs.tolist()))
    want = set(map(tuple, KR.kdtree_pairs(pos, dirs, r, min_cos, bidir).tolist()))
    odd = np.array(sorted(got ^ want), np.int64).reshape(-1, 2)
    both = np.array(sorted(got | want), np.int64).reshape(-1, 2)
    assert KR.pairs_excused(pos, dirs, r, min_cos, odd).all(), (name, len(odd))
    n_exc = int(KR.pairs_excused(pos, dirs, r, min_cos, both).sum())
    print(f"KNN_PAIRS {name} pairs={len(got)} differing={len(odd)} excused={n_exc} of {len(both)}")
    assert len(pairs) == len(got) >= 1 and (pairs[:, 0] < pairs[:, 1]).all()
    if not on_lattice:                              # the float32 statement cannot drift unnoticed: the excuse covers < 1 % of a case
        assert n_exc < 0.01 * len(both)
    if name == "dense_ball":
        assert len(got) == 600 * 599 // 2 > 4 * 600                     # the callers' first capacity overflows
    if name == "identical_300":
        assert np.all(dist == 0)
    if name == "blob_2":
        assert pairs.tolist() == [[0, 1]] and dist[0] == np.float32(r)          # the smallest size is a hit, on equality
    if name == "x_planes":
        r2 = np.float32(r) * np.float32(r)
        d = pos[pairs[:, 0]] - pos[pairs[:, 1]]
        assert int((((d * d).sum(1) == r2) & (d[:, 0] != 0)).sum()) == 9 * 300    # a partner at exactly the radius on each neighbouring plane
    if name == "on_the_radius":
        d = pos[pairs[:, 0]] - pos[pairs[:, 1]]
        dot = -(dirs[pairs[:, 0]] * dirs[pairs[:, 1]]).sum(1)
        assert ((d * d).sum(1) == np.float32(r) ** 2).sum() > 100 and (dot == np.float32(min_cos)).sum() > 100


def test_merge_cluster_has_more_candidates_than_the_first_capacity():
    """The premise of the model-level GPU test, from the model's own defaults (arguments.OptimizationParams)."""
    from arguments import OptimizationParams
    opt = OptimizationParams()
    pts, _ = KC.merge_cluster_strands()
    tips = pts[:, 2]
    dirs = pts[:, 1] - tips
    dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    pairs, _ = KR.brute_pairs_f32(tips, dirs, opt.merge_dist_th_init, np.cos(np.deg2rad(opt.merge_angle_th_init)), True)
    n_ends = 2 * pts.shape[0]
    assert len(pairs) == 64 * 63 // 2 > max(4 * n_ends, 1024)
    d = np.linalg.norm(tips - np.array([0.2, 0.3, 0.1]), axis=1)
    assert d.max() <= 0.25 * opt.merge_dist_th_init * 1.001


# ---- which input catches which decision of distCUDA2's grid search: the CPU port with single decisions switched off ----------
_PORT_CASES = ["margin_cloud"] + KC.NAMES


def _port_case(name):
    if name == "margin_cloud":
        p = KC.margin_cloud()
        return p, KR.brute_dist2_f32(p)
    return _small(name)


def _port_diff(name, flags):
    p, ref = _port_case(name)
    got, left = O.dist2_grid(p, flags)
    return int((_bits(got) != _bits(ref)).sum()), left


@pytest.mark.parametrize("name", _PORT_CASES)
def test_grid_port_as_written_equals_brute_force(name):
    assert _port_diff(name, 0) == (0, 0)


def test_grid_port_without_the_margin():
    """Only the constructed cloud needs the 1.000001f: point 0 and its two copies lose their third neighbour."""
    p, ref = _port_case("margin_cloud")
    got, left = O.dist2_grid(p, O.GRID_NO_MARGIN)
    assert left == 0 and np.nonzero(_bits(got) != _bits(ref))[0].tolist() == [0, 1, 2]
    for name in KC.NAMES:
        assert _port_diff(name, O.GRID_NO_MARGIN) == (0, 0), name


def test_grid_port_without_the_own_cell_guard():
    """The own cell walked twice: every family with a non-zero third distance differs."""
    for name in _PORT_CASES:
        diff, left = _port_diff(name, O.GRID_NO_OWN_GUARD)
        assert left == 0 and (diff > 0) == (name not in ("all_same", "all_origin", "dup5")), (name, diff)


def test_grid_port_without_the_clamp():
    """Without min(..., 1023u) a cube range leaves the grid wherever an extent is zero or tiny, or a radius passes the box."""
    for name in ("plane_z0", "line", "aniso", "clusters", "margin_cloud"):
        diff, left = _port_diff(name, O.GRID_NO_CLAMP)
        assert left > 0, (name, diff, left)


def test_sorted_early_exit_decided_on_equality():
    """radius_pairs_kernel's tile walk on the x_planes case, in numpy: with `>` no pair is lost, with `>=` the partners at
    exactly the radius in a tile that starts on block_max_x are."""
    pos, dirs, r, min_cos, bidir, _ = KC.pair_cases()["x_planes"]
    pairs, _ = KR.brute_pairs_f32(pos, dirs, r, min_cos, bidir)
    order = np.argsort(pos[:, 0], kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    xs, N = pos[order, 0], pos.shape[0]
    a, b = rank[pairs].min(axis=1), rank[pairs].max(axis=1)
    lost = {}
    for strict in (True, False):
        lost[strict] = 0
        for blk in range((N + 255) // 256):
            block_max_x = np.float32(xs[min(N - 1, blk * 256 + 255)] + np.float32(r))
            stop = N
            for t0 in range(blk * 256, N, 256):
                if (xs[t0] > block_max_x) if strict else (xs[t0] >= block_max_x):
                    stop = t0
                    break
            lost[strict] += int((b[a // 256 == blk] >= stop).sum())
    print(f"KNN_EARLY_EXIT lost with >: {lost[True]}, with >=: {lost[False]} of {len(pairs)}")
    assert lost[True] == 0 and lost[False] > 100


def test_knn3_tile_ties_reference():
    p = KC.knn3_tile_ties()
    d2, idx = KR.brute_knn3_f32(p)
    assert idx[254:259].tolist() == [[254, 255, 256]] * 5 and idx[510:515].tolist() == [[510, 511, 512]] * 5
    assert np.all(d2[254:259] == 0) and np.all(d2[510:515] == 0)


@pytest.mark.parametrize("n", [3, 4, 255, 513])
def test_knn3_self_cpu_branch_keeps_the_non_finite_contract(n):
    """loss.losses.knn3_self on CPU tensors: the row of a point with a non-finite coordinate is (-1, +inf) three times, such a
    point appears in no other row, and everything equals the float32 brute force bit for bit."""
    import torch
    from loss.losses import knn3_self
    if n <= 4:
        p = KC.non_finite(n, 7, rows=(1,))              # two or three finite points: fewer than three comparable candidates
    else:
        p = KC.knn3_case("non_finite", n)
    bad = ~np.isfinite(p).all(axis=1)
    d2, idx = knn3_self(torch.from_numpy(p))
    d2, idx = d2.numpy(), idx.numpy()
    rd2, ridx = KR.brute_knn3_f32(p)
    assert (idx[bad] == -1).all() and np.isposinf(d2[bad]).all()
    assert not np.isin(idx, np.nonzero(bad)[0]).any()
    assert np.array_equal(idx, ridx) and np.array_equal(_bits(d2), _bits(rd2))


@pytest.mark.parametrize("name", KC.KNN3_FAMILIES)
def test_knn3_self_cpu_branch_equals_brute_force(name):
    import torch
    from loss.losses import knn3_self
    p = KC.knn3_case(name, 513)
    d2, idx = knn3_self(torch.from_numpy(p))
    rd2, ridx = KR.brute_knn3_f32(p)
    assert np.array_equal(idx.numpy(), ridx) and np.array_equal(_bits(d2.numpy()), _bits(rd2))


def test_nearest_cases_need_float64():
    """The inputs of the hgs_nearest_distance_f64 test: a float32 evaluation of the same expression gets them wrong."""
    pts, refs = KC.nearest_case(257, 1025)
    want = KR.brute_nearest_f64(pts, refs)
    d = pts[:, None, :] - refs.astype(np.float32)[None, :, :]
    f32 = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1))
    assert (want == 0).sum() >= 80 and (f32.astype(np.float64) != want).sum() > 10
    far = 255
    assert np.linalg.norm(pts[far]) > 1e4 and abs(want[far] - 0.01) < 1e-10      # (the runner-up is 1e-9 farther)
