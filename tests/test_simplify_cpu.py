"""The strand simplification on the CPU (scene/strand_simplify.py numpy path, export_strands.py --simplify): the round-by-round path
against the recursive restatement of the contract (tests/simplify_reference.py) bit for bit on the cases of tests/simplify_cases.py,
the contract's consequences (every dropped joint within tol of its final segment, the bits that must not change, idempotence, tol = 0),
the report on a hand-worked strand, the parameter check, the C entry point's refusals (which launch nothing) and the driver.  Every
comparison is of bytes or of integers; no numeric tolerance is involved but in the hand-worked report, whose expected figures are
decimal fractions."""
import functools
import math

import numpy as np
import pytest

from tests import simplify_cases as SC
from tests import simplify_reference as SR


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of one hard case: (keep, status, rounds); computed once, shared with the GPU tests."""
    return SR.simplify(*SC.hard_cases()[name])


def assert_same(got, ref, what):
    for name, a, b in zip(("keep", "status", "rounds"), got, ref):
        assert SR.same_bytes(np.asarray(a), b), (what, name)


def cut(ref, off, K):
    """The first K strands of a result: strands are independent."""
    return ref[0][:off[K]], ref[1][:K], ref[2][:K]


def export_of(pts, off, attrs=None):
    from scene.strand_export import StrandExport
    K = off.shape[0] - 1
    attrs = np.zeros((pts.shape[0], 1), np.float32) if attrs is None else attrs
    return StrandExport(pts, attrs, off, np.arange(K, dtype=np.int64) + 5, np.zeros(K))


@pytest.mark.parametrize("name", SC.HARD_NAMES)
def test_numpy_path_matches_the_recursive_restatement(name):
    from scene.strand_simplify import simplify_numpy
    got = simplify_numpy(*SC.hard_cases()[name])
    assert_same(got, reference(name), name)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32 and got[2].dtype == np.int32


@pytest.mark.parametrize("K", SC.KS)
def test_numpy_path_at_every_strand_count(K):
    from scene.strand_simplify import simplify_numpy
    pts, off, tol = SC.hard_cases()["pool"]
    p, o = SC.first_strands(pts, off, K)
    assert_same(simplify_numpy(p, o, tol), cut(reference("pool"), off, K), f"K={K}")


def test_the_cases_exercise_what_they_are_meant_to():
    """The restatement's own results say that every branch of the contract is taken."""
    keep, status, rounds = reference("edges")
    assert status.tolist() == [1 if n < 3 else 2 if n > 1024 else 0 for n in SC.EDGE_N]
    assert rounds[SC.EDGE_N.index(3)] in (0, 1) and rounds[SC.EDGE_N.index(1025)] == 0 and rounds[SC.EDGE_N.index(1024)] > 10
    _, off, _ = SC.hard_cases()["edges"]
    assert keep[off[-2]:].all() and 0 < keep[off[-3]:off[-2]].sum() < 1024        # the LONG strand whole, the last eligible one thinned
    assert reference("nonfinite")[1].tolist() == [0, 3] * 5 and not reference("nonfinite")[2][1::2].any()
    keep, status, rounds = reference("shapes")
    _, off, _ = SC.hard_cases()["shapes"]
    kept = lambda name: np.nonzero(keep[off[SC.shape_index(name)]:off[SC.shape_index(name) + 1]])[0].tolist()
    assert kept("straddle") == [0, 60, 70, 129]                                   # the interval (60, 70) lies across lanes 63 | 64
    assert 64 in kept("straddle_bump") and {0, 60, 70, 129} < set(kept("straddle_bump"))
    assert kept("collinear") == [0, 128] and rounds[SC.shape_index("collinear")] == 0
    assert kept("square") == [0, 1, 2, 3, 4]                                      # a == b: the distance to the point a
    assert len(kept("closed_loop")) > 6 and kept("hairpin")[:2] == [0, 10]
    # the hairpin's joints clamp at both ends of the chord from the root to the tip
    pts = SC.shape_strands()[0][off[SC.shape_index("hairpin")]:off[SC.shape_index("hairpin") + 1]].astype(np.float64)
    ts = [SR.deviation2(p, pts[0], pts[-1])[1] for p in pts[1:-1]]
    assert 0.0 in ts and 1.0 in ts and any(0.0 < t < 1.0 for t in ts)
    keep0, _, rounds0 = reference("shapes_tol0")
    assert keep0[off[SC.shape_index("collinear")]:off[SC.shape_index("collinear") + 1]].sum() == 2     # tol = 0 drops what has d2 == 0
    # the tie rule decides: somewhere a later joint shares the winner's d2
    pts, off, tol = SC.hard_cases()["ties"]
    ties = 0
    for s in range(off.shape[0] - 1):
        p = pts[off[s]:off[s + 1]].astype(np.float64)
        if len(p) >= 4:
            d2 = [SR.deviation2(q, p[0], p[-1])[0] for q in p[1:-1]]
            ties += d2.count(max(d2)) > 1 and max(d2) > tol * tol
    assert ties >= 20
    keep, _, rounds = reference("chain")
    assert keep.all() and rounds.tolist() == [34]                                 # n - 2 deep: every split is next to the left end
    assert 2 < reference("chain_tol")[0].sum() < 36
    assert reference("pool")[1][9] == 3 and (reference("pool")[1] == 0).sum() > 250 and reference("mixed")[2].max() > 20


@pytest.mark.parametrize("name", SC.HARD_NAMES)
def test_consequences_of_the_contract(name):
    """Every dropped joint lies within tol of its final segment (d2 <= tol*tol by the contract's statement: no slack), roots, tips and
    the strands that are not OK keep every joint, and simplifying the result again keeps everything."""
    from scene.strand_simplify import simplify_numpy, simplify_strands
    pts, off, tol = SC.hard_cases()[name]
    keep, status, rounds = simplify_numpy(pts, off, tol)
    n = off[1:] - off[:-1]
    assert keep[off[:-1][n > 0]].all() and keep[(off[1:] - 1)[n > 0]].all()
    for s in np.nonzero(status != 0)[0]:
        assert keep[off[s]:off[s + 1]].all() and rounds[s] == 0
    worst = 0.0
    for r, d2, t, left, right in SR.final_deviations(pts, off, keep):
        assert d2 <= tol * tol, (name, r, d2)
        worst = max(worst, d2)
    print(f"{name}: tol {tol:g}, largest deviation of a dropped joint {math.sqrt(worst):.6g}")
    if tol == 0.0:
        assert worst == 0.0
    attrs = np.arange(pts.shape[0] * 2, dtype=np.float32).reshape(-1, 2)
    res, rep = simplify_strands(export_of(pts, off, attrs), tol)
    sel = keep != 0
    assert SR.same_bytes(res.points, pts[sel]) and SR.same_bytes(res.attrs, attrs[sel])       # kept joints: their input bits
    assert np.array_equal(res.offsets[1:] - res.offsets[:-1], np.add.reduceat(np.append(keep, 0).astype(np.int64), off[:-1]) * (n > 0))
    assert rep["largest_deviation"] == math.sqrt(worst) and rep["joints_after"] == int(sel.sum())
    again = simplify_numpy(res.points, res.offsets, tol)
    assert again[0].all() and SR.same_bytes(again[2], rounds), name                 # idempotent: the same splits again, and nothing to drop


def test_simplify_strands_reports_on_a_hand_worked_strand():
    """tests/simplify_cases.py WORKED, tol = 0.5: joint 2 is kept at depth 1 (d2 = 1), joints 1 and 3 are dropped with d2 = 0.2 at
    t = 0.4 and t = 0.6.  Attribute 0 is the joint's number, linear along the strand but not along the new segments: 1 against
    0 + 0.4 * 2 = 0.8 and 3 against 2 + 0.6 * 2 = 3.2; attribute 1 is constant."""
    from scene.strand_collide import strand_lengths
    from scene.strand_simplify import simplify_strands
    nan = [[0, 0, 0], [1, np.nan, 0], [2, 0, 0]]
    pts, off = SC._pack([SC.WORKED, [[5, 5, 5], [6, 6, 6]], nan, np.zeros((1025, 3)), [], [[0, 0, 0], [1, 0, 0], [2, 0, 0]]])
    attrs = np.stack([np.arange(pts.shape[0]) - 0.0, np.full(pts.shape[0], 7.0)], axis=1).astype(np.float32)
    strands = export_of(pts, off, attrs)
    res, rep = simplify_strands(strands, 0.5)
    assert res.points[:3].tolist() == [[0, 0, 0], [2, 1, 0], [4, 0, 0]] and res.attrs[:3, 0].tolist() == [0.0, 2.0, 4.0]
    assert res.offsets.tolist() == [0, 3, 5, 8, 1033, 1033, 1035] and res.offsets.dtype == np.int64
    assert np.array_equal(res.strand_ids, strands.strand_ids)
    with np.errstate(invalid="ignore"):
        assert SR.same_bytes(res.length, strand_lengths(res.points, res.offsets)) and res.length[0] == 2.0 * math.sqrt(5.0) and res.length[5] == 2.0
    assert set(rep) == {"strands", "ok", "short", "long", "nonfinite", "joints_before", "joints_after", "ratio", "kept_min", "kept_mean",
                        "kept_max", "rounds_max", "largest_deviation", "attr_deviation"}
    assert (rep["strands"], rep["ok"], rep["short"], rep["long"], rep["nonfinite"]) == (6, 2, 2, 1, 1)
    assert (rep["joints_before"], rep["joints_after"], rep["kept_min"], rep["kept_max"], rep["rounds_max"]) == (1038, 1035, 2, 3, 1)
    assert rep["ratio"] == 1035 / 1038 and rep["kept_mean"] == 2.5
    assert abs(rep["largest_deviation"] - math.sqrt(0.2)) < 1e-15 and len(rep["attr_deviation"]) == 2
    assert abs(rep["attr_deviation"][0] - 0.2) < 1e-12 and rep["attr_deviation"][1] == 0.0
    res, rep = simplify_strands(strands, 1.0)                                      # 1 > 1 is false: joint 2 goes too
    assert res.offsets.tolist() == [0, 2, 4, 7, 1032, 1032, 1034] and rep["largest_deviation"] == 1.0 and rep["rounds_max"] == 0
    assert rep["attr_deviation"][0] == 0.0                                         # (the joint's number is linear along the chord)


def test_parameters_are_checked():
    from scene.strand_simplify import check_parameters, simplify_numpy, simplify_strands
    for bad in SC.REFUSED:
        with pytest.raises(ValueError, match="tol"):
            check_parameters(bad)
    assert check_parameters(0) == 0.0 and check_parameters(np.float32(0.5)) == 0.5 and isinstance(check_parameters(1), float)
    pts, off = SC.shape_strands()
    with pytest.raises(ValueError, match="tol"):
        simplify_numpy(pts, off, -1.0)
    for bad in (off[1:], off[:-1], off[::-1].copy(), off.astype(np.float64)):
        with pytest.raises(ValueError, match="offsets"):
            simplify_numpy(pts, bad, 0.5)
    with pytest.raises(ValueError, match="points"):
        simplify_numpy(pts.reshape(-1), off, 0.5)
    with pytest.raises(ValueError, match="device"):
        simplify_strands(export_of(pts, off), 0.5, device="cpu")


def test_take_strands_follows_the_index_order():
    from scene.strand_simplify import take_strands
    pts, off = SC.shape_strands()
    strands = export_of(pts, off, np.arange(pts.shape[0], dtype=np.float32)[:, None])
    got = take_strands(strands, [4, 0, 5])
    assert got.offsets.tolist() == [0, 129, 259, 264] and got.strand_ids.tolist() == [9, 5, 10]
    assert SR.same_bytes(got.points, np.concatenate([pts[off[4]:off[5]], pts[off[0]:off[1]], pts[off[5]:off[6]]]))
    assert got.attrs[129, 0] == 0.0 and got.attrs[0, 0] == float(off[4])


# ---- the entry point's refusals ------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments():
    """Nothing is launched: these run without a GPU (non-null arguments are the addresses of host buffers that are never read)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    bufs = [C.create_string_buffer(64) for _ in range(5)]
    off, pts, keep, st, rd = (C.addressof(b) for b in bufs)
    nan, inf = float("nan"), float("inf")

    def call(K=2, P=5, offsets=off, points=pts, max_joints=3, tol=0.5, k=keep, status=st, rounds=rd):
        code = L.hgs_strand_simplify(None, K, offsets, P, points, max_joints, tol, k, status, rounds)
        return code, L.hgs_last_error().decode()

    for kw, words in ((dict(K=-1), "bad sizes"), (dict(P=-1), "bad sizes"), (dict(max_joints=-1), "max_joints"), (dict(max_joints=1), "max_joints"),
                      (dict(max_joints=2), "max_joints"), (dict(max_joints=1025), "max_joints"), (dict(tol=-1.0), "tol"), (dict(tol=nan), "tol"),
                      (dict(tol=inf), "tol"), (dict(tol=-inf), "tol"), (dict(offsets=None), "null"), (dict(points=None), "null"),
                      (dict(k=None), "null"), (dict(status=None), "null"), (dict(rounds=None), "null"), (dict(k=pts), "alias"),
                      (dict(rounds=st), "alias"), (dict(status=off), "alias")):
        code, msg = call(**kw)
        assert code == 1 and "hgs_strand_simplify" in msg and words in msg, (kw, msg)
    # nothing to do is not an error, and no pointer is looked at; a bad tolerance is refused even then
    assert L.hgs_strand_simplify(None, 0, None, 0, None, 0, 0.0, None, None, None) == 0
    assert call(K=0, tol=nan)[0] == 1 and call(K=0, max_joints=2)[0] == 1


# ---- the driver --------------------------------------------------------------------------------------------------------------------
DRIVER_TOL = "2e-4"


def test_driver_simplifies_the_strands(tmp_path, capsys):
    import export_strands
    from data import strand_files as F
    from data.cy_hair import read_cy_hair
    from scene.strand_simplify import simplify_strands
    from tests.test_collide_cpu import driver_scene
    model, field = driver_scene(tmp_path)
    common = ["-m", str(model), "--device", "cpu", "--format", "hair", "--format", "usc"]
    for points in ("20", "0"):                                                    # resampled, and the joints as they are (ragged)
        capsys.readouterr()
        plain, pp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"plain{points}")])
        assert "Simplified strands" not in capsys.readouterr().out
        F.write_strands_cy(str(tmp_path / "was.hair"), plain)                      # without the flag: the bytes the writers give the chain's strands
        F.write_strands_usc(str(tmp_path / "was.data"), plain)
        assert open(pp["hair"], "rb").read() == open(tmp_path / "was.hair", "rb").read()
        assert open(pp["usc"], "rb").read() == open(tmp_path / "was.data", "rb").read()
        res, rp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"simple{points}"), "--simplify", DRIVER_TOL])
        text = capsys.readouterr().out
        line = [t for t in text.splitlines() if t.startswith("Simplified strands (tol 0.0002): ")]
        want, rep = simplify_strands(plain, float(DRIVER_TOL))
        assert len(line) == 1 and f"{rep['joints_after']} of {rep['joints_before']} joints kept" in line[0]
        assert text.index("Simplified strands") < text.index("Saved hair")
        assert 2 * plain.n_strands < rep["joints_after"] < rep["joints_before"] and rep["ok"] >= 5
        assert SR.same_bytes(res.points, want.points) and SR.same_bytes(res.attrs, want.attrs) and SR.same_bytes(res.offsets, want.offsets)
        assert SR.same_bytes(res.length, want.length) and np.array_equal(res.strand_ids, plain.strand_ids)
        # the ragged files, read back by the project's own readers: the simplified counts
        hair = read_cy_hair(rp["hair"])
        cnt = want.offsets[1:] - want.offsets[:-1]
        assert np.array_equal(hair.segments.astype(np.int64) + 1, cnt) and SR.same_bytes(hair.points, want.points)
        assert SR.same_bytes(hair.thickness, want.attrs[:, 4]) and SR.same_bytes(hair.colors, want.attrs[:, :3])
        pts, off = F.read_usc_hair(rp["usc"])
        assert SR.same_bytes(pts, want.points) and SR.same_bytes(off, want.offsets)
        assert len(np.unique(cnt)) > 1
    # the flag comes last in the chain's order
    chain = common + ["--points", "20", "--head_sdf", str(field), "--attach_roots", "--smooth_strands", "--interpolate", "--guides", "3", "--resolve_head"]
    off_, _ = export_strands.main(chain + ["-o", str(tmp_path / "chain_off")])
    capsys.readouterr()
    on, _ = export_strands.main(chain + ["-o", str(tmp_path / "chain_on"), "--simplify", DRIVER_TOL])
    text = capsys.readouterr().out
    marks = [text.index(w) for w in ("Attached to the head", "Smoothed strands", "Interpolated:", "Resolved against the head", "Simplified strands", "Saved hair")]
    assert marks == sorted(marks) and text.count("Simplified strands") == 1
    want, _ = simplify_strands(off_, float(DRIVER_TOL))
    assert SR.same_bytes(on.points, want.points) and SR.same_bytes(on.offsets, want.offsets) and on.points.shape[0] < off_.points.shape[0]


def test_driver_simplifies_the_guides_and_keeps_the_binding(tmp_path, capsys):
    import export_strands
    from data import strand_files as F
    from scene.strand_simplify import simplify_strands, take_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    common = ["-m", str(model), "--device", "cpu", "--points", "9", "--format", "hair", "--format", "usc", "--interpolate", "--select_guides", "5",
              "--select_samples", "4", "--select_iters", "6"]
    plain, pp = export_strands.main(common + ["-o", str(tmp_path / "plain")])
    capsys.readouterr()
    res, rp = export_strands.main(common + ["-o", str(tmp_path / "simple"), "--simplify", DRIVER_TOL])
    text = capsys.readouterr().out
    assert text.index("Selected guides") < text.index("Simplified strands") < text.index("Saved hair")       # chosen first, on the uniform strands
    want, rep = simplify_strands(plain, float(DRIVER_TOL))
    assert SR.same_bytes(res.points, want.points) and rep["joints_after"] < rep["joints_before"]
    with np.load(pp["guide_binding"]) as a, np.load(rp["guide_binding"]) as b:
        assert set(a.files) == set(b.files)
        for key in a.files:
            assert SR.same_bytes(a[key], b[key]), key
        guide_strand = a["guide_strand"]
    guides = take_strands(want, guide_strand)
    F.write_strands_cy(str(tmp_path / "want.hair"), guides)
    F.write_strands_usc(str(tmp_path / "want.data"), guides)
    assert open(rp["hair_guides"], "rb").read() == open(tmp_path / "want.hair", "rb").read()
    assert open(rp["usc_guides"], "rb").read() == open(tmp_path / "want.data", "rb").read()
    pts, off = F.read_usc_hair(rp["usc_guides"])
    for g, s in enumerate(guide_strand):
        assert SR.same_bytes(pts[off[g]:off[g + 1]], want.points[want.offsets[s]:want.offsets[s + 1]])


def test_driver_refuses_bad_values(tmp_path, capsys):
    import export_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    for bad in ("-1", "nan", "inf", "-inf"):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), f"--simplify={bad}"])
        assert stop.value.code == 2 and "export_strands.py: --simplify" in capsys.readouterr().err, bad
    with pytest.raises(SystemExit) as stop:                                        # (argparse's own refusal of a word that is no number)
        export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), "--simplify", "wide"])
    assert stop.value.code == 2
    assert not (tmp_path / "x.hair").exists()
