"""The strand smoothing on the CPU (scene/strand_smooth.py numpy path, export_strands.py --smooth_strands): the vectorised path
against the loop restatement of the contract (tests/smooth_reference.py) bit for bit on the cases of tests/smooth_cases.py, the bits
that must not change, what the filter is for (asserted on the restatement and on the product), the parameter check, the report, the
C entry point's refusals (which launch nothing) and the driver."""
import functools
import math

import numpy as np
import pytest

from tests import smooth_cases as SC
from tests import smooth_reference as SR


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of one hard case: (out, status, clamped); computed once, shared with the GPU tests."""
    pts, off, params = SC.hard_cases()[name]
    return SR.smooth(pts, off, *params)


@functools.lru_cache(maxsize=None)
def pool_reference():
    """The restatement of the 257-strand pool; strands are independent, so its first K strands are the case of K strands."""
    return SR.smooth(*SC.pool_strands(), *SC.DEFAULTS)


def assert_same(got, ref, what):
    for name, a, b in zip(("points", "status", "clamped"), got, ref):
        assert SR.same_bytes(np.asarray(a), b), (what, name)


def strand(arrays, off, s):
    return arrays[off[s]:off[s + 1]]


def test_the_case_names_are_the_cases():
    assert tuple(SC.hard_cases()) == SC.HARD_NAMES


@pytest.mark.parametrize("name", SC.HARD_NAMES)
def test_numpy_path_matches_the_loop_restatement(name):
    from scene.strand_smooth import smooth_numpy
    pts, off, params = SC.hard_cases()[name]
    got = smooth_numpy(pts, off, *params)
    assert_same(got, reference(name), name)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32


@pytest.mark.parametrize("K", SC.KS)
def test_numpy_path_at_every_strand_count(K):
    from scene.strand_smooth import smooth_numpy
    pts, off = SC.first_strands(*SC.pool_strands(), K)
    ref = pool_reference()
    assert_same(smooth_numpy(pts, off, *SC.DEFAULTS), (ref[0][:off[K]], ref[1][:K], ref[2][:K]), f"K={K}")


def test_the_cases_exercise_what_they_are_meant_to():
    """The restatement's own results say that every branch of the contract is taken."""
    _, status, _ = reference("edges_default")
    assert status.tolist() == [1 if n < 3 else 2 if n > 1024 else 0 for n in SC.EDGE_N]
    out, status, clamped = reference("special_default")
    pts, off = SC.special_strands()
    want = [3 if name in ("nan_middle", "inf_middle", "nan_end", "inf_end") else 0 for name in SC.SPECIAL]
    assert status.tolist() == want and not clamped.any()
    s = SC.special_index("collapsed")
    assert SR.same_bytes(out[off[s] + 1], pts[off[s] + 1])                       # both neighbours equal and s_j == 0: the joint stays
    assert not SR.same_bytes(out[off[s] + 3], pts[off[s] + 3])
    s = SC.special_index("collapsed_beside_long")
    assert not SR.same_bytes(strand(out, off, s), strand(pts, off, s))
    _, _, clamped = reference("special_move")
    n_zig = int(off[SC.special_index("zigzag") + 1] - off[SC.special_index("zigzag")])
    assert clamped[SC.special_index("zigzag")] > (n_zig - 2) // 2                # most of the zigzag's joints are held
    assert clamped[SC.special_index("line")] == 0
    assert reference("edges_move")[2].sum() > 0 and reference("mixed_move")[2].sum() > 0
    assert pool_reference()[1][9] == 3 and (pool_reference()[1] == 0).sum() > 200
    assert not SR.same_bytes(reference("special_mu0")[0], out) and not SR.same_bytes(reference("special_i1")[0], out)
    assert np.isfinite(reference("special_i256")[0][off[SC.special_index("far")]:]).all()


@pytest.mark.parametrize("name", SC.HARD_NAMES)
def test_bits_that_must_not_change(name):
    from scene.strand_smooth import smooth_numpy
    pts, off, params = SC.hard_cases()[name]
    for out, status, _ in (smooth_numpy(pts, off, *params), reference(name)):
        copied = 0
        for s in range(off.shape[0] - 1):
            a, b = int(off[s]), int(off[s + 1])
            if b == a:
                continue
            assert SR.same_bytes(out[a], pts[a]) and SR.same_bytes(out[b - 1], pts[b - 1]), s      # the root and the tip
            if status[s] != 0:
                assert SR.same_bytes(out[a:b], pts[a:b]), s                       # SHORT / LONG / NONFINITE: every bit
                copied += 1
            else:
                assert np.isfinite(out[a:b]).all()
        assert copied == int((status != 0).sum() - (off[1:] == off[:-1]).sum())


# ---- what the filter is for: on the restatement, and on the product -------------------------------------------------------------------
def both(points, params):
    """The smoothed strand [n, 3] by the restatement and by the numpy path."""
    from scene.strand_smooth import smooth_numpy
    pts = np.asarray(points, np.float32)
    off = np.array([0, pts.shape[0]], np.int64)
    return SR.smooth(pts, off, *params), smooth_numpy(pts, off, *params)


def test_the_noisy_arc_gets_smoother_and_keeps_its_length():
    arc, clean = SC.noisy_arc().astype(np.float32), SR.polyline_length(SC.clean_arc().astype(np.float32))
    for res in both(arc, SC.DEFAULTS):
        before, after = SR.turning_angle(arc), SR.turning_angle(res[0])
        print(f"noisy arc: mean turning angle {before:.4g} -> {after:.4g} degrees")
        assert after < before
    for taubin, laplace in zip(both(arc, (50, 0.5, -0.53, None)), both(arc, (50, 0.5, 0.0, None))):
        lt, ll = SR.polyline_length(taubin[0]), SR.polyline_length(laplace[0])
        print(f"noisy arc, 50 iterations: clean length {clean:.6g}, lambda|mu {lt:.6g}, lambda alone {ll:.6g}")
        assert abs(lt - clean) < abs(ll - clean)


def test_a_straight_line_stays():
    line = SC.straight_line().astype(np.float32)
    ulp = float(np.spacing(np.abs(line).max()))                                 # one float32 unit in the last place of the largest coordinate
    for res in both(line, SC.DEFAULTS):
        worst = float(np.abs(res[0].astype(np.float64) - line.astype(np.float64)).max())
        print(f"straight line: largest change of a coordinate {worst:.3g}, one ulp of the largest coordinate {ulp:.3g}")
        assert worst <= ulp


def test_max_move_bounds_every_displacement():
    """|x_j - p_j| <= D after the clamp up to the float64 rounding of four operations (relative 1e-15, taken as 1e-12); the float32
    rounding of the output moves each coordinate by at most half a unit in the last place of the written value."""
    D = SC.ZIGZAG_MOVE
    for name in ("special_move", "edges_move", "mixed_move"):
        pts, off, params = SC.hard_cases()[name]
        assert params[3] == D
        from scene.strand_smooth import smooth_numpy
        for out, status, _ in (reference(name), smooth_numpy(pts, off, *params)):
            with np.errstate(invalid="ignore"):
                disp = np.linalg.norm(out.astype(np.float64) - pts.astype(np.float64), axis=1)
                bound = D * (1.0 + 1e-12) + np.sqrt(((0.5 * np.spacing(np.abs(out)).astype(np.float64)) ** 2).sum(axis=1))
            ok = np.isfinite(disp)
            print(f"{name}: largest displacement {disp[ok].max():.9g} for D = {D:g}, largest excess over D {float((disp[ok] - D).max()):.3g}, "
                  f"allowed {float(bound[ok].max() - D):.3g}")
            assert (disp[ok] <= bound[ok]).all() and disp[ok].max() > 0.9 * D


def test_the_zigzag_is_flattened():
    """The zigzag is the operator's highest mode (eigenvalue 2): a lambda sweep with lambda = 0.5 multiplies it by 1 - 2*0.5 = 0 in the
    interior; what is left comes from the pinned ends.  137 degrees must fall below 10."""
    zig = SC.zigzag().astype(np.float32)
    for res in both(zig, SC.DEFAULTS):
        before, after = SR.turning_angle(zig), SR.turning_angle(res[0])
        print(f"zigzag: mean turning angle {before:.4g} -> {after:.4g} degrees")
        assert 130.0 < before < 140.0 and after < 10.0


# ---- arguments, report -------------------------------------------------------------------------------------------------------------
def test_parameters_are_checked():
    from scene.strand_smooth import check_parameters, smooth_numpy, smooth_strands
    from scene.strand_export import StrandExport
    for params, words in SC.REFUSED:
        with pytest.raises(ValueError, match=words):
            check_parameters(*params)
    for params in SC.PARAMS.values():
        assert check_parameters(*params) == (params[0], params[1], params[2], params[3])
    assert check_parameters() == SC.DEFAULTS
    pts, off = SC.special_strands()
    with pytest.raises(ValueError, match="iters"):
        smooth_numpy(pts, off, iters=0)
    for bad in (off[1:], off[:-1], off[::-1].copy(), off.astype(np.float64)):
        with pytest.raises(ValueError, match="offsets"):
            smooth_numpy(pts, bad)
    with pytest.raises(ValueError, match="points"):
        smooth_numpy(pts.reshape(-1), off)
    strands = StrandExport(pts, np.zeros((pts.shape[0], 1), np.float32), off, np.arange(off.shape[0] - 1, dtype=np.int64), np.zeros(off.shape[0] - 1))
    with pytest.raises(ValueError, match="device"):
        smooth_strands(strands, device="cpu")


def test_smooth_strands_reports_and_recomputes_the_length():
    """A right-angled corner of two segments of length sqrt(2), one sweep with lambda = 0.5: a = b = 0.5, m = (1, 0, 0), the corner
    moves from (1, 1, 0) to (1, 0.5, 0): by 0.5, the turn from 90 degrees to 2 atan(0.5), the length from 2 sqrt(2) to 2 sqrt(1.25)."""
    from scene.strand_collide import strand_lengths
    from scene.strand_export import StrandExport
    from scene.strand_smooth import smooth_strands
    corner = [[0, 0, 0], [1, 1, 0], [2, 0, 0]]
    nan = [[0, 0, 0], [1, np.nan, 0], [2, 0, 0]]
    pts, off = SC._pack([corner, [[5, 5, 5], [6, 6, 6]], nan, np.zeros((1025, 3)), []])
    K = off.shape[0] - 1
    attrs = np.arange(pts.shape[0] * 2, dtype=np.float32).reshape(-1, 2)
    strands = StrandExport(pts, attrs, off, np.arange(K, dtype=np.int64) + 5, np.zeros(K))
    res, rep = smooth_strands(strands, iters=1, lam=0.5, mu=0.0)
    assert res.points[1].tolist() == [1.0, 0.5, 0.0] and SR.same_bytes(np.delete(res.points, 1, axis=0), np.delete(pts, 1, axis=0))
    assert res.attrs is attrs and res.offsets is off and np.array_equal(res.strand_ids, strands.strand_ids)
    with np.errstate(invalid="ignore"):
        assert SR.same_bytes(res.length, strand_lengths(res.points, off)) and res.length[0] == 2.0 * math.sqrt(1.25)
    assert set(rep) == {"strands", "smoothed", "short", "long", "nonfinite", "joints", "clamped", "largest_displacement", "mean_displacement",
                        "turning_before", "turning_after", "length_ratio_min", "length_ratio_mean", "length_ratio_max"}
    assert (rep["strands"], rep["smoothed"], rep["short"], rep["long"], rep["nonfinite"], rep["joints"], rep["clamped"]) == (5, 1, 2, 1, 1, 1033, 0)
    assert rep["largest_displacement"] == rep["mean_displacement"] == 0.5
    assert abs(rep["turning_before"] - 90.0) < 1e-9 and abs(rep["turning_after"] - math.degrees(2.0 * math.atan(0.5))) < 1e-9
    ratio = math.sqrt(1.25) / math.sqrt(2.0)
    assert all(abs(rep[k] - ratio) < 1e-12 for k in ("length_ratio_min", "length_ratio_mean", "length_ratio_max"))
    res, rep = smooth_strands(strands, iters=1, lam=0.5, mu=0.0, max_move=0.25)
    assert res.points[1].tolist() == [1.0, 0.75, 0.0] and rep["clamped"] == 1 and rep["largest_displacement"] == 0.25


# ---- the entry point's refusals ------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments():
    """Nothing is launched: these run without a GPU (non-null arguments are the addresses of host buffers that are never read)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    bufs = [C.create_string_buffer(64) for _ in range(5)]
    off, pts, out, st, cl = (C.addressof(b) for b in bufs)
    nan, inf = float("nan"), float("inf")

    def call(K=2, P=5, offsets=off, points=pts, max_joints=3, iters=10, lam=0.5, mu=-0.53, has=0, move=0.0, o=out, status=st, clamped=cl):
        code = L.hgs_strand_smooth(None, K, offsets, P, points, max_joints, iters, lam, mu, has, move, o, status, clamped)
        return code, L.hgs_last_error().decode()

    for kw, words in ((dict(K=-1), "bad sizes"), (dict(P=-1), "bad sizes"), (dict(max_joints=-1), "bad sizes"), (dict(max_joints=1025), "bad sizes"),
                      (dict(iters=0), "iters = 0"), (dict(iters=257), "iters = 257"), (dict(lam=0.0), "lam"), (dict(lam=1.5), "lam"),
                      (dict(lam=nan), "lam"), (dict(lam=1.0, mu=-1.0), "mu"), (dict(mu=-0.5), "mu"), (dict(mu=0.3), "mu"), (dict(mu=-1.01), "mu"),
                      (dict(mu=nan), "mu"), (dict(lam=0.9, mu=-1.0), "grow"), (dict(has=1, move=0.0), "max_move"), (dict(has=1, move=-1.0), "max_move"),
                      (dict(has=1, move=inf), "max_move"), (dict(has=1, move=nan), "max_move"), (dict(offsets=None), "null"),
                      (dict(points=None), "null"), (dict(o=None), "null"), (dict(status=None), "null"), (dict(clamped=None), "null"),
                      (dict(o=pts), "alias"), (dict(clamped=st), "alias")):
        code, msg = call(**kw)
        assert code == 1 and "hgs_strand_smooth" in msg and words in msg, (kw, msg)
    # nothing to do is not an error, and no pointer is looked at; bad parameters are refused even then
    assert L.hgs_strand_smooth(None, 0, None, 0, None, 0, 1, 0.5, 0.0, 0, nan, None, None, None) == 0
    assert call(K=0, iters=0)[0] == 1 and call(K=0, lam=2.0)[0] == 1


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def test_driver_smooths_the_strands(tmp_path, capsys):
    import export_strands
    from data import strand_files as F
    from scene.strand_smooth import smooth_strands
    from tests.test_collide_cpu import driver_scene
    model, field = driver_scene(tmp_path)
    common = ["-m", str(model), "--device", "cpu", "--format", "hair", "--format", "usc"]
    for points in ("20", "0"):                                                    # resampled, and the joints as they are (ragged)
        capsys.readouterr()
        plain, pp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"plain{points}")])
        assert "Smoothed strands" not in capsys.readouterr().out
        # without the flag its knobs change nothing: the files are what they were before there was a flag
        _, kp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"knobs{points}"), "--smooth_iters", "3", "--smooth_lambda",
                                              "0.9", "--smooth_mu", "0", "--smooth_max_move", "1e-4"])
        for f in ("hair", "usc"):
            assert open(pp[f], "rb").read() == open(kp[f], "rb").read()
        capsys.readouterr()
        res, rp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"smooth{points}"), "--smooth_strands", "--smooth_iters", "5"])
        text = capsys.readouterr().out
        line = [t for t in text.splitlines() if t.startswith("Smoothed strands")]
        want, rep = smooth_strands(plain, iters=5)
        assert len(line) == 1 and f"{rep['smoothed']} of {rep['strands']} strands smoothed" in line[0] and rep["smoothed"] >= 5
        assert SR.same_bytes(res.points, want.points) and SR.same_bytes(res.length, want.length) and res.attrs.tobytes() == plain.attrs.tobytes()
        assert np.array_equal(res.offsets, plain.offsets) and not SR.same_bytes(res.points, plain.points)
        assert SR.same_bytes(res.points[res.offsets[:-1]], plain.points[plain.offsets[:-1]])          # every root
        assert SR.same_bytes(res.points[res.offsets[1:] - 1], plain.points[plain.offsets[1:] - 1])    # every tip
        F.write_strands_cy(str(tmp_path / "want.hair"), want)
        F.write_strands_usc(str(tmp_path / "want.data"), want)
        assert open(rp["hair"], "rb").read() == open(tmp_path / "want.hair", "rb").read() != open(pp["hair"], "rb").read()
        assert open(rp["usc"], "rb").read() == open(tmp_path / "want.data", "rb").read() != open(pp["usc"], "rb").read()
    # the flag composes with the rest of the chain, in the chain's order: attach, smooth, interpolate, resolve
    chain = common + ["--points", "20", "--head_sdf", str(field), "--attach_roots", "--interpolate", "--guides", "3", "--resolve_head"]
    off_, _ = export_strands.main(chain + ["-o", str(tmp_path / "chain_off")])
    capsys.readouterr()
    on, _ = export_strands.main(chain + ["-o", str(tmp_path / "chain_on"), "--smooth_strands", "--smooth_max_move", "1e-3"])
    text = capsys.readouterr().out
    marks = [text.index(w) for w in ("Attached to the head", "Smoothed strands", "Interpolated:", "Resolved against the head")]
    assert marks == sorted(marks) and text.count("Smoothed strands") == 1 and " held at 0.001, " in text
    assert on.n_strands == off_.n_strands and np.array_equal(on.offsets, off_.offsets) and not SR.same_bytes(on.points, off_.points)


def test_driver_refuses_bad_values(tmp_path, capsys):
    import export_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    for bad in (["--smooth_iters", "0"], ["--smooth_iters", "257"], ["--smooth_lambda", "0"], ["--smooth_lambda", "1.5"], ["--smooth_mu", "-0.4"],
                ["--smooth_mu", "0.2"], ["--smooth_lambda", "1", "--smooth_mu", "-1"], ["--smooth_lambda", "0.9", "--smooth_mu", "-1"],
                ["--smooth_max_move", "0"], ["--smooth_max_move", "-1"], ["--smooth_max_move", "nan"]):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), "--smooth_strands"] + bad)
        assert stop.value.code == 2 and "export_strands.py: --smooth_strands" in capsys.readouterr().err, bad
    assert not (tmp_path / "x.hair").exists()
