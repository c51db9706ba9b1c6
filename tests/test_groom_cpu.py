"""The groom interpolation on the CPU (scene/groom.py numpy path, export_strands.py --interpolate): the vectorised path against the
loop restatement of the contract (tests/groom_reference.py) bit for bit on the size grid and the hard inputs (tests/groom_cases.py),
the interpolation's quality on an analytic groom, the driver, and the entry points' refusals (which launch nothing)."""
import functools
import os

import numpy as np
import pytest

from tests import groom_cases as GC
from tests import groom_reference as GR
from tests import strand_export_reference as R


def _cos_max(angle):
    from scene.groom import search_parameters
    return search_parameters(None, angle)[1]


def assert_search_equal(got, ref, what):
    for name, a, b in zip(("idx", "d2", "w", "count"), got, ref):
        assert GR.same_bytes(np.asarray(a), b), (what, name)


@functools.lru_cache(maxsize=None)
def reference_blend(case):
    """The restatement of one BLEND_CASES entry: (search tuple, points, attrs, kept, length); computed once, shared with the GPU tests."""
    N, K, k, M, C, max_d2, angle = case
    gp, ga, roots = GC.grid_case(K, M, C)
    roots = roots[:N]
    cands, ch = GR.grid_candidates(K)
    s = GR.search(cands[:N], ch, k, max_d2, _cos_max(angle))
    pts, att, kept = GR.blend(gp, ga, roots, s[0], s[2], s[3])
    return s, pts, att, kept, GR.lengths(pts, M)


@pytest.mark.parametrize("K", GC.KS)
def test_numpy_search_matches_the_loop_restatement(K):
    from scene.groom import search_numpy
    gp, _, roots = GC.grid_case(K)
    cands, ch = GR.grid_candidates(K)
    dropped = 0
    for k in GC.KNN:
        for max_d2 in GC.MAX_D2:
            for angle in GC.ANGLES:
                ref = GR.search(cands, ch, k, max_d2, _cos_max(angle))
                dropped += int((ref[3] == 0).sum())
                for N in GC.NS:
                    got = search_numpy(gp, roots[:N], k, max_d2, _cos_max(angle))
                    assert_search_equal(got, tuple(a[:N] for a in ref), f"K={K} k={k} max_d2={max_d2} angle={angle} N={N}")
    assert dropped > 0


def test_the_grid_exercises_what_it_is_meant_to():
    """Ties, d2 == 0, d2 == max_d2 and every kind of dropped guide occur in the grid's inputs (the restatement's own lists say so)."""
    cands, ch = GR.grid_candidates(513)
    ties = sum(1 for c in cands for a, b in zip(c, c[1:4]) if a[0] == b[0])
    assert ties > 100 and sum(1 for c in cands if c and c[0][0] == 0.0) > 20
    assert sum(1 for c in cands for d2, _ in c if d2 == 4.0) > 100
    assert sum(1 for c in cands if not c) == 4                                  # the NaN, inf and 1e200 roots
    assert all(g not in (2, 4) for c in cands for _, g in c)                    # the guides with a NaN / infinite root
    full = GR.search(cands, ch, 8, np.inf, -2.0)[3]
    part = GR.search(cands, ch, 8, np.inf, _cos_max(60.0))[3]
    assert (part < full).sum() > 100 and sum(1 for c in ch if c[3] == 0.0) > 40 and sum(1 for c in ch if c[3] != c[3]) == 2
    few = GR.search(cands, ch, 8, 1.0, -2.0)[3]
    print("counts at max_d2 = 1:", np.bincount(few, minlength=9).tolist())
    assert (few == 0).sum() >= 4 and (few == 1).sum() > 20 and ((few > 1) & (few < 8)).sum() > 20
    none = GR.search(*GR.grid_candidates(7), 8, 1.0, -2.0)[3]
    assert (none == 0).sum() > 100


@pytest.mark.parametrize("case", GC.hard_cases(), ids=lambda c: c[0])
def test_hard_inputs(case):
    from scene.groom import blend_numpy, search_numpy
    name, gp, ga, roots, k, max_d2, angle, expect = case
    cos_max = _cos_max(angle)
    ref = GR.search(GR.candidates(gp, roots), GR.chords(gp), k, max_d2, cos_max)
    got = search_numpy(gp, roots, k, max_d2, cos_max)
    assert_search_equal(got, ref, name)
    if expect is not None:
        assert [[int(g) for g in row if g >= 0] for row in got[0]] == expect and got[3].tolist() == [len(e) for e in expect]
    kept = np.nonzero(got[3] > 0)[0]
    pts, att = blend_numpy(gp, ga, roots, got[0], got[2], kept)
    rp, ra, rk = GR.blend(gp, ga, roots, ref[0], ref[2], ref[3])
    assert np.array_equal(kept, rk) and GR.same_bytes(pts, rp) and GR.same_bytes(att, ra), name


def test_hard_input_values():
    """What the rules mean in numbers, on the hand-built cases."""
    from scene.groom import search_numpy
    cases = {c[0]: c for c in GC.hard_cases()}
    _, gp, _, roots, k, max_d2, angle, _ = cases["ties"]
    idx, d2, w, count = search_numpy(gp, roots, k, max_d2, _cos_max(angle))
    assert d2[0].tolist() == [1.0, 1.0, 1.0] and w[0].tolist() == [1.0 / 3.0] * 3
    assert d2[1].tolist() == [0.0, np.inf, np.inf] and w[1].tolist() == [1.0, 0.0, 0.0] and idx[1].tolist() == [0, -1, -1]
    assert d2[2].tolist() == [1.0, 2.0, 2.0] and w[2].tolist() == [1.0 / 2.0, 0.5 / 2.0, 0.5 / 2.0]
    _, gp, _, roots, k, max_d2, angle, _ = cases["radius 9"]
    idx, d2, w, count = search_numpy(gp, roots, k, max_d2, _cos_max(angle))
    assert d2[0].tolist() == [1.0, 4.0, 9.0, np.inf] and count.tolist() == [3, 2, 1, 0] and idx[3].tolist() == [-1] * 4
    W = (1.0 + 0.25) + 1.0 / 9.0
    assert w[0].tolist() == [1.0 / W, 0.25 / W, (1.0 / 9.0) / W, 0.0]


@pytest.mark.parametrize("case", GC.BLEND_CASES, ids=lambda c: "N{}-K{}-k{}-M{}-C{}".format(*c[:5]))
def test_numpy_path_matches_the_loop_restatement(case):
    from scene.groom import interpolate_strands
    from scene.strand_export import StrandExport
    N, K, k, M, C, max_d2, angle = case
    gp, ga, roots = GC.grid_case(K, M, C)
    guides = StrandExport(gp.reshape(-1, 3), ga.reshape(-1, C), np.arange(K + 1, dtype=np.int64) * M, np.arange(K, dtype=np.int64), np.zeros(K))
    res = interpolate_strands(guides, roots[:N], k=k, max_guide_distance=None if np.isinf(max_d2) else float(np.sqrt(max_d2)), max_angle=angle,
                              first_id=1000)
    s, pts, att, kept, length = reference_blend(case)
    assert float(np.sqrt(max_d2)) ** 2 == max_d2                                # (the distance the driver would be given squares to the case's max_d2)
    assert np.array_equal(res.root_ids, kept) and res.n_dropped == N - kept.shape[0]
    assert GR.same_bytes(res.strands.points, pts) and GR.same_bytes(res.strands.attrs, att)
    assert GR.same_bytes(res.strands.length, length) and GR.same_bytes(res.n_guides, s[3][kept])
    assert np.array_equal(res.strands.offsets, np.arange(kept.shape[0] + 1) * M) and np.array_equal(res.strands.strand_ids, 1000 + kept)
    # point 0 of every strand is its root rounded to float32
    with np.errstate(all="ignore"):
        assert GR.same_bytes(res.strands.points[::M], roots[:N][kept].astype(np.float32))


def test_arguments_are_checked():
    from scene.groom import interpolate_strands, search_parameters
    from scene.strand_export import StrandExport
    gp, ga, roots = GC.grid_case(7, 3, 2)
    guides = StrandExport(gp.reshape(-1, 3), ga.reshape(-1, 2), np.arange(8, dtype=np.int64) * 3, np.arange(7, dtype=np.int64), np.zeros(7))
    assert np.array_equal(interpolate_strands(guides, roots[:9]).strands.strand_ids, 7 + np.array([0, 1, 2, 4, 6, 8]))   # (roots 3, 5 and 7 are not finite)
    ragged = guides._replace(offsets=np.array([0, 2, 6, 9, 12, 15, 18, 21], np.int64))
    with pytest.raises(ValueError, match="native mode"):
        interpolate_strands(ragged, roots)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="k = "):
            interpolate_strands(guides, roots, k=bad)
    with pytest.raises(ValueError, match="device"):
        interpolate_strands(guides, roots, device="cpu")
    with pytest.raises(ValueError, match="max_guide_distance"):
        interpolate_strands(guides, roots, max_guide_distance=float("nan"))
    with pytest.raises(ValueError, match="roots"):
        interpolate_strands(guides, roots.reshape(-1))
    assert search_parameters(3.0, 180.0) == (9.0, -2.0) and search_parameters(None, 0.0) == (np.inf, 1.0)
    assert search_parameters(None, 60.0)[1] == np.cos(np.radians(60.0))


def test_interpolation_quality_on_an_analytic_groom():
    """Every tenth strand of an analytic groom is a guide, the rest the truth: blending 4 guides must come closer than copying 1."""
    from scene.groom import interpolate_strands
    from scene.strand_export import StrandExport
    roots, truth = GC.analytic_groom(2000, 17)
    is_guide = np.arange(2000) % 10 == 0
    gp = truth[is_guide].astype(np.float32)
    K = gp.shape[0]
    guides = StrandExport(gp.reshape(-1, 3), np.zeros((K * 17, 1), np.float32), np.arange(K + 1, dtype=np.int64) * 17, np.arange(K, dtype=np.int64),
                          np.zeros(K))
    err = {}
    for k in (1, 4):
        res = interpolate_strands(guides, roots[~is_guide], k=k, max_guide_distance=None, max_angle=60.0)
        assert res.n_dropped == 0
        err[k] = float(np.linalg.norm(res.strands.points.reshape(-1, 17, 3).astype(np.float64) - truth[~is_guide], axis=2).mean())
    print(f"mean point error: k=1 {err[1]:.5f}, k=4 {err[4]:.5f}, ratio {err[4] / err[1]:.3f}")
    assert err[4] < 0.7 * err[1]


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def driver_model(tmp_path):
    """A model directory of 7 strands whose file carries 7 x 3 + 1 strand roots: every strand's own root, two more a millimetre beside
    it, and one far from all of them.  Returns (directory, number of roots)."""
    m = R.mixed_model([5, 40, 64, 65, 130, 1, 17], device="cpu", seed=21)
    own = np.asarray(m.ref_strand_root, np.float64)
    rng = np.random.default_rng(5)
    extra = np.concatenate([own + 1e-3 * rng.normal(size=own.shape), own + 1e-3 * rng.normal(size=own.shape), [[0.0, 0.0, 5.0]]])
    m.ref_strand_root = np.concatenate([own, extra])
    m.compute_strands_info()
    assert m.strands_info.n_strands == 7
    model = tmp_path / "out"
    os.makedirs(model / "point_cloud" / "iteration_9")
    m.save_ply(str(model / "point_cloud" / "iteration_9" / "point_cloud.ply"))
    return model, 22


def test_driver_interpolates(tmp_path, capsys):
    import export_strands
    from data.cy_hair import read_cy_hair
    model, n_roots = driver_model(tmp_path)
    common = ["-m", str(model), "--device", "cpu", "--points", "9", "--format", "hair", "--format", "ply_edges", "--colour", "strand"]
    plain, _ = export_strands.main(common + ["-o", str(tmp_path / "plain")])
    capsys.readouterr()
    res, paths = export_strands.main(common + ["-o", str(tmp_path / "groom"), "--interpolate", "--max_guide_distance", "0.5"])
    text = capsys.readouterr().out
    assert f"Interpolated: {n_roots} roots, 1 dropped" in text and "21 strands from 7 guides" in text and "guides per root" in text
    hf = read_cy_hair(paths["hair"])
    assert hf.header.hair_count == 7 + 21 and np.all(hf.segments == 8) and hf.points.shape[0] == 28 * 9
    assert np.array_equal(hf.points[:63], plain.points) and np.array_equal(res.strand_ids, np.concatenate([np.arange(7), 7 + np.arange(21)]))
    # a root that IS a guide's root copies that guide
    assert np.array_equal(hf.points[63:63 + 63], plain.points) and np.array_equal(res.attrs[63:126], plain.attrs)
    only, paths = export_strands.main(common + ["-o", str(tmp_path / "only"), "--interpolate", "--no_guides", "--roots", "11", "--guides", "2"])
    text = capsys.readouterr().out
    assert "Interpolated: 11 roots, 0 dropped" in text
    hf = read_cy_hair(paths["hair"])
    assert hf.header.hair_count == 11 and np.all(hf.segments == 8) and np.array_equal(only.strand_ids, 7 + np.arange(11))
    with pytest.raises(SystemExit) as stop:
        export_strands.main(common[:4] + ["-o", str(tmp_path / "x"), "--points", "0", "--interpolate"])
    assert stop.value.code == 2
    err = capsys.readouterr().err
    assert "export_strands.py: --interpolate" in err and "--points 0" in err


def test_driver_counts_points_inside_the_head(tmp_path, capsys):
    """With -s the roots are the capture's scalp points, and where the capture has a distance field of the head the driver says how
    many interpolated points lie inside it (and writes them all the same)."""
    import export_strands
    from data.head_reconstruction_data import save_head_reconstruction_data_npz
    from utils import head_sdf
    model, _ = driver_model(tmp_path)
    m = R.mixed_model([5, 40, 64, 65, 130, 1, 17], device="cpu", seed=21)
    own = np.asarray(m.ref_strand_root, np.float64)
    scalp = np.concatenate([own, 0.5 * own, [[0.0, 0.0, 0.0]]])                 # the strands' own roots, and roots deep inside the head
    capture = tmp_path / "capture"
    os.makedirs(capture)
    save_head_reconstruction_data_npz(str(capture / "head_reconstruction_data.npz"), scalp, scalp)
    verts = 0.09 * np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
    faces = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.int64)
    sdf = head_sdf.build_sdf(verts, faces, grid=16, pad=0.5)
    head_sdf.save_sdf(str(capture / head_sdf.FILE), sdf)
    res, _ = export_strands.main(["-m", str(model), "-s", str(capture), "-o", str(tmp_path / "g"), "--device", "cpu", "--points", "9",
                                  "--interpolate", "--no_guides"])
    text = capsys.readouterr().out
    assert "Interpolated: 15 roots, 0 dropped" in text and res.n_strands == 15
    _, _, d, in_range = head_sdf.sample(res.points, head_sdf.load_sdf(str(capture / head_sdf.FILE)))
    inside = int(np.count_nonzero(in_range & (d < 0)))
    assert 8 <= inside < res.points.shape[0] and f"{inside} of {15 * 9} interpolated points" in text


# ---- the entry points' refusals ------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    """Nothing is launched: these run without a GPU (non-null arguments are the address of a host buffer that is never read)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    inf = float("inf")

    def nb(N=4, K=3, M=3, k=4, max_d2=inf, cos_max=0.5, roots=p, gp=p, idx=p, d2=p, w=p, count=p):
        status = L.hgs_groom_neighbours(None, N, roots, K, M, gp, k, max_d2, cos_max, idx, d2, w, count)
        return status, L.hgs_last_error().decode()

    def bl(K=3, M=3, C_=2, k=4, n_kept=2, gp=p, ga=p, roots=p, idx=p, w=p, kept=p, op=p, oa=p):
        status = L.hgs_groom_blend(None, K, M, C_, gp, ga, roots, k, idx, w, n_kept, kept, op, oa)
        return status, L.hgs_last_error().decode()

    for kw, words in ((dict(k=0), "k = 0"), (dict(k=9), "k = 9"), (dict(M=1), "M = 1"), (dict(N=-1), "bad sizes"), (dict(K=-1), "bad sizes"),
                      (dict(max_d2=float("nan")), "NaN"), (dict(roots=None), "null"), (dict(gp=None), "null"), (dict(idx=None), "null"),
                      (dict(d2=None), "null"), (dict(w=None), "null"), (dict(count=None), "null")):
        status, msg = nb(**kw)
        assert status == 1 and "hgs_groom_neighbours" in msg and words in msg, (kw, msg)
    for kw, words in ((dict(k=0), "k = 0"), (dict(k=9), "k = 9"), (dict(M=1), "M = 1"), (dict(C_=0), "C = 0"), (dict(C_=17), "C = 17"),
                      (dict(K=-1), "bad sizes"), (dict(n_kept=-1), "bad sizes"), (dict(M=65536, n_kept=32768), "2^31"), (dict(K=0), "no guide"),
                      (dict(gp=None), "null"), (dict(ga=None), "null"), (dict(roots=None), "null"), (dict(idx=None), "null"),
                      (dict(w=None), "null"), (dict(kept=None), "null"), (dict(op=None), "null"), (dict(oa=None), "null")):
        status, msg = bl(**kw)
        assert status == 1 and "hgs_groom_blend" in msg and words in msg, (kw, msg)
    # nothing to do is not an error, and no argument is looked at
    assert L.hgs_groom_neighbours(None, 0, None, 0, 2, None, 1, inf, -2.0, None, None, None, None) == 0
    assert L.hgs_groom_blend(None, 0, 2, 1, None, None, None, 1, None, None, 0, None, None, None) == 0
