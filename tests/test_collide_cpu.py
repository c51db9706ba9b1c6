"""The head push-out on the CPU (scene/strand_collide.py numpy path, export_strands.py --resolve_head): the vectorised path against
the loop restatement of the contract (tests/collide_reference.py) bit for bit on the hard cases of tests/collide_cases.py, an analytic
head that every strand must leave, segment lengths to the rounding of the float32 endpoints, the bits that must not change, the
driver, and the C entry point's refusals (which launch nothing)."""
import functools
import os

import numpy as np
import pytest

from tests import collide_cases as CC
from tests import collide_reference as CR


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of one hard case: (out, moved, unresolved, first_hit); computed once, shared with the GPU tests."""
    pts, off, fname, margin, skin, iters = CC.hard_cases()[name]
    return CR.resolve(pts, off, CC.field(fname), margin, skin, iters)


@functools.lru_cache(maxsize=None)
def counted_reference():
    """The restatement of the 1000-strand case; strands are independent, so its first K strands are the case of K strands."""
    pts, off = CC.counted_strands()
    fname, margin, skin, iters = CC.COUNTED
    return CR.resolve(pts, off, CC.field(fname), margin, skin, iters)


def assert_same(got, ref, what):
    for name, a, b in zip(("points", "moved", "unresolved"), got, ref):
        assert CR.same_bytes(np.asarray(a), b), (what, name)


def inside(points, sdf, margin):
    """bool [P]: in range and d < margin, by the product's own sampling statement."""
    from utils.head_sdf import trilinear
    ok, d, _, _, _ = trilinear(points, sdf)
    with np.errstate(invalid="ignore"):
        return ok & (d < np.float32(margin))


def test_the_case_names_are_the_cases():
    assert tuple(CC.hard_cases()) == CC.HARD_NAMES


@pytest.mark.parametrize("name", CC.HARD_NAMES)
def test_numpy_path_matches_the_loop_restatement(name):
    from scene.strand_collide import resolve_numpy
    pts, off, fname, margin, skin, iters = CC.hard_cases()[name]
    got = resolve_numpy(pts, off, CC.field(fname), margin, skin, iters)
    assert_same(got, reference(name)[:3], name)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32


@pytest.mark.parametrize("K", CC.KS)
def test_numpy_path_at_every_strand_count(K):
    from scene.strand_collide import resolve_numpy
    fname, margin, skin, iters = CC.COUNTED
    pts, off = CC.first_strands(*CC.counted_strands(), K)
    ref = counted_reference()
    got = resolve_numpy(pts, off, CC.field(fname), margin, skin, iters)
    assert_same(got, (ref[0][:off[K]], ref[1][:K], ref[2][:K]), f"K={K}")


def test_the_cases_exercise_what_they_are_meant_to():
    """The restatement's own results say that every branch of the contract is taken."""
    out, moved, unresolved, first = reference("special_m0.0_sNone_i8")
    pts, off = CC.special_strands()
    n = off[1:] - off[:-1]
    assert moved[0] > 0 and unresolved[0] == 0                                   # through the head: pushed out
    assert moved[1] > moved[0]                                                   # twice
    assert unresolved[2] > 0 and unresolved[3] > 0                               # a root inside holds its first joints inside
    assert not np.isfinite(out[off[7]:off[8]]).all() and moved[7] > 0            # the NaN joint behind a hit
    assert moved[10] == 1 and moved[11] == 1                                     # out of range counts as outside
    assert CR.same_bytes(out[off[8]:off[8] + 3], pts[off[8]:off[8] + 3])         # an inf joint before any hit is written as it is
    assert moved[12] >= 2 and unresolved[12] == 0                                # the centre node has a gradient: the cell's forward difference
    assert (n[16:20] < 2).all() and not moved[16:20].any() and not unresolved[16:20].any()
    assert CR.same_bytes(out[off[16]:off[20]], pts[off[16]:off[20]])             # strands of 0 and 1 joints are copied, a NaN included
    _, moved1, unresolved1, _ = reference("special_m0.0_sNone_i1")
    assert unresolved1.sum() > unresolved.sum()                                  # one push is not enough behind a moved joint
    _, m_r, _, f_r = reference("ragged")
    assert (m_r > 0).sum() > 20 and (m_r == 0).sum() > 10
    out_f, moved_f, unresolved_f, _ = reference("flat")
    assert moved_f.tolist() == [0, 2] and unresolved_f.tolist() == [3, 0]        # zero gradient: the joints stay inside and are counted
    fp, fo = CC.flat_strands()
    assert CR.same_bytes(out_f[:fo[1]], fp[:fo[1]])
    ref = counted_reference()
    assert 300 < (ref[1] > 0).sum() < 700


# ---- the analytic head --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sphere_result(grid, margin, iters):
    from scene.strand_collide import resolve_numpy
    pts, off = CC.sphere_scene()
    return resolve_numpy(pts, off, CC.field(f"sphere{grid}"), margin, None, iters)


@pytest.mark.parametrize("grid", CC.SPHERE_GRIDS)
@pytest.mark.parametrize("margin", CC.SPHERE_MARGINS)
@pytest.mark.parametrize("iters", CC.SPHERE_ITERS)
def test_every_strand_leaves_the_analytic_head(grid, margin, iters):
    pts, off = CC.sphere_scene()
    sdf = CC.field(f"sphere{grid}")
    out, moved, unresolved = sphere_result(grid, margin, iters)
    before, after = int(inside(pts, sdf, margin).sum()), int(inside(out, sdf, margin).sum())
    print(f"grid {grid} margin {margin} iters {iters}: inside before {before}, after {after}, moved {int(moved.sum())}, unresolved {int(unresolved.sum())}")
    assert before > 0 and not inside(pts[off[:-1]], sdf, margin).any()          # (the roots are outside: nothing holds a joint inside)
    assert int(unresolved.sum()) == 0 and after == 0
    assert moved.sum() >= before


def segment_bound(a, b):
    """What the rounding of two float32 endpoints allows a segment's length to change by: every coordinate of an endpoint is off by at
    most half a unit in its last place, so the segment's vector by at most the sum of the two per coordinate; and a relative 1e-12
    for the float64 arithmetic that placed the joint (a few hundred times its rounding)."""
    ha, hb = (0.5 * np.spacing(np.abs(v)).astype(np.float64) for v in (a, b))
    return np.sqrt(((ha + hb) ** 2).sum(axis=1))


def test_segment_lengths_are_kept():
    pts, off = CC.sphere_scene()
    worst = 0.0
    for grid in CC.SPHERE_GRIDS:
        for margin in CC.SPHERE_MARGINS:
            out = sphere_result(grid, margin, 8)[0]
            seg = np.ones(pts.shape[0] - 1, bool)
            seg[off[1:-1] - 1] = False                                           # (between two strands)
            a, b = out[:-1][seg], out[1:][seg]
            got = np.linalg.norm(b.astype(np.float64) - a.astype(np.float64), axis=1)
            want = np.linalg.norm(pts[1:][seg].astype(np.float64) - pts[:-1][seg].astype(np.float64), axis=1)
            bound = segment_bound(a, b) + 1e-12 * want
            worst = max(worst, float((np.abs(got - want) / want).max()))
            assert (np.abs(got - want) <= bound).all(), (grid, margin, float((np.abs(got - want) - bound).max()))
    print(f"largest relative change of a segment's length: {worst:.3g}")


@pytest.mark.parametrize("name", ("special_m0.05_sNone_i8", "ragged", "slab_margin"))
def test_bits_that_must_not_change(name):
    from scene.strand_collide import resolve_numpy
    pts, off, fname, margin, skin, iters = CC.hard_cases()[name]
    sdf = CC.field(fname)
    out, moved, _ = resolve_numpy(pts, off, sdf, margin, skin, iters)
    was_inside = inside(pts, sdf, margin)
    kept = 0
    for s in range(off.shape[0] - 1):
        a, b = int(off[s]), int(off[s + 1])
        if b == a:
            continue
        assert CR.same_bytes(out[a], pts[a])                                     # the root
        behind = np.nonzero(was_inside[a + 1:b])[0]                              # joints behind the root that start inside
        first = a + 1 + int(behind[0]) if behind.size else b
        assert CR.same_bytes(out[a:first], pts[a:first]), s                      # every joint before the strand's first hit
        assert (moved[s] == 0) == (behind.size == 0), s                          # a strand is touched iff a joint behind its root is inside
        kept += behind.size == 0
    assert kept >= 3 and (moved > 0).sum() >= 3
    assert np.array_equal(reference(name)[3] + off[:-1] >= off[1:], moved == 0)


def test_resolve_head_reports_and_recomputes_the_length():
    from scene.groom import polyline_length
    from scene.strand_collide import resolve_head, strand_lengths
    from scene.strand_export import StrandExport
    pts, off = CC.sphere_scene()
    K = off.shape[0] - 1
    attrs = np.arange(pts.shape[0] * 2, dtype=np.float32).reshape(-1, 2)
    strands = StrandExport(pts, attrs, off, np.arange(K, dtype=np.int64) + 5, np.zeros(K))
    sdf = CC.field("sphere32")
    res, stats = resolve_head(strands, sdf, margin=0.02)
    out, moved, unresolved = sphere_result(32, 0.02, 8)
    assert CR.same_bytes(res.points, out) and res.attrs is attrs and res.offsets is off and np.array_equal(res.strand_ids, strands.strand_ids)
    assert CR.same_bytes(res.length, polyline_length(out.reshape(K, 32, 3)))
    assert stats["joints"] == pts.shape[0] and stats["inside_before"] == int(inside(pts, sdf, 0.02).sum()) and stats["inside_after"] == 0
    assert stats["moved"] == int(moved.sum()) and stats["unresolved"] == 0 and stats["strands_touched"] == int((moved > 0).sum())
    assert stats["deepest_before"] > 0.02 and stats["deepest_after"] == 0.0
    assert 0.02 < stats["largest_displacement"] == float(np.linalg.norm(out.astype(np.float64) - pts.astype(np.float64), axis=1).max())
    # ragged strands: the length of each is its own polyline's, 0 without a segment
    rp, ro = CC.ragged_strands()
    length = strand_lengths(rp, ro)
    for s in (0, 1, 2, 3, 7, ro.shape[0] - 2):
        n = int(ro[s + 1] - ro[s])
        assert length[s] == (polyline_length(rp[ro[s]:ro[s + 1]].reshape(1, n, 3))[0] if n >= 2 else 0.0)


def test_arguments_are_checked():
    from scene.strand_collide import resolve_head, resolve_numpy
    from scene.strand_export import StrandExport
    from utils.head_sdf import HeadSDF
    pts, off = CC.flat_strands()
    sdf = CC.field("flat")
    for kw, words in ((dict(margin=-0.1), "margin"), (dict(margin=np.nan), "margin"), (dict(margin=np.inf), "margin"), (dict(skin=-1.0), "skin"),
                      (dict(skin=np.nan), "skin"), (dict(iters=0), "iters"), (dict(iters=33), "iters"), (dict(iters=2.5), "iters")):
        with pytest.raises(ValueError, match=words):
            resolve_numpy(pts, off, sdf, **kw)
    for bad in (off[1:], off[:-1], off[::-1].copy(), np.array([0, 7, 5, 9]), off.astype(np.float64)):
        with pytest.raises(ValueError, match="offsets"):
            resolve_numpy(pts, bad, sdf)
    with pytest.raises(ValueError, match="points"):
        resolve_numpy(pts.reshape(-1), off, sdf)
    with pytest.raises(ValueError, match="at least 2"):
        resolve_numpy(pts, off, HeadSDF(np.zeros(3), 1.0, (3, 1, 2), np.zeros((2, 1, 3), np.float32)))
    strands = StrandExport(pts, np.zeros((pts.shape[0], 1), np.float32), off, np.arange(2, dtype=np.int64), np.zeros(2))
    with pytest.raises(ValueError, match="device"):
        resolve_head(strands, sdf, device="cpu")


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def driver_scene(tmp_path):
    """(model directory, field file): the 7-strand model of the groom tests, and an analytic ball that its strands pass through."""
    import export_strands
    from tests.test_groom_cpu import driver_model
    from utils import head_sdf
    model, _ = driver_model(tmp_path)
    plain, _ = export_strands.main(["-m", str(model), "--device", "cpu", "--points", "9", "-o", str(tmp_path / "probe")])
    lo, hi = plain.points.min(axis=0).astype(np.float64), plain.points.max(axis=0).astype(np.float64)
    mids = plain.points.reshape(-1, 9, 3)[:, 4].astype(np.float64)
    centre = mids[np.argsort(np.linalg.norm(mids - mids.mean(axis=0), axis=1))[0]]               # on a strand, in the middle of them
    radius = 0.25 * float(np.linalg.norm(hi - lo))
    origin, h, grid = lo - 0.2 * (hi - lo).max(), 1.4 * (hi - lo).max() / 23, 24
    z, y, x = np.meshgrid(*(origin[k] + h * np.arange(grid) for k in (2, 1, 0)), indexing="ij")
    phi = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    path = tmp_path / "field" / head_sdf.FILE
    os.makedirs(path.parent)
    head_sdf.save_sdf(str(path), head_sdf.HeadSDF(origin, h, (grid, grid, grid), phi.astype(np.float32)))
    return model, path


def test_driver_resolves_the_head(tmp_path, capsys):
    import export_strands
    from data import strand_files as F
    from scene.strand_collide import resolve_head
    from scene.strand_export import resample_strands
    from utils import head_sdf
    from utils.system import model_ply
    model, field = driver_scene(tmp_path)
    sdf = head_sdf.load_sdf(str(field))
    common = ["-m", str(model), "--device", "cpu", "--format", "hair", "--format", "usc"]
    for points in ("9", "0"):                                                     # resampled, and the joints as they are (ragged)
        capsys.readouterr()
        plain, pp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"plain{points}")])
        assert "Resolved against the head" not in capsys.readouterr().out
        # without the flag the files are the writers' bytes of the resampled strands: what they were before there was a flag
        m = export_strands.load_strand_model(model_ply(str(model)), None, device="cpu")
        direct = resample_strands(m, points=int(points), min_segments=1, min_length=0.0, max_root_distance=None, device=None)
        F.write_strands_cy(str(tmp_path / "direct.hair"), direct)
        F.write_strands_usc(str(tmp_path / "direct.data"), direct)
        assert open(pp["hair"], "rb").read() == open(tmp_path / "direct.hair", "rb").read()
        assert open(pp["usc"], "rb").read() == open(tmp_path / "direct.data", "rb").read()
        res, rp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"res{points}"), "--resolve_head", "--head_sdf", str(field),
                                               "--head_margin", "0.001", "--collide_iters", "6"])
        text = capsys.readouterr().out
        want, stats = resolve_head(plain, sdf, margin=0.001, iters=6)
        assert stats["inside_before"] > 3 and stats["moved"] >= stats["inside_before"] - 7 and stats["strands_touched"] > 0
        assert CR.same_bytes(res.points, want.points) and CR.same_bytes(res.length, want.length) and res.attrs.tobytes() == plain.attrs.tobytes()
        assert not CR.same_bytes(res.points, plain.points) and np.array_equal(res.offsets, plain.offsets)
        assert f"inside the head before: {stats['inside_before']} of {stats['joints']} points, after: {stats['inside_after']}" in text
        assert f"moved {stats['moved']} points of {stats['strands_touched']} strands" in text and f"unresolved: {stats['unresolved']}" in text
        assert "largest displacement" in text
        F.write_strands_cy(str(tmp_path / "want.hair"), want)
        assert open(rp["hair"], "rb").read() == open(tmp_path / "want.hair", "rb").read() != open(pp["hair"], "rb").read()


def test_driver_resolves_interpolated_strands_and_finds_the_capture_field(tmp_path, capsys):
    """With -s the field is the capture's head_sdf.npz; the push-out runs over the guides and the interpolated strands, after the
    interpolation; the count of points inside the head is printed only when they are written as they are."""
    import shutil
    import export_strands
    from data.head_reconstruction_data import save_head_reconstruction_data_npz
    from tests import strand_export_reference as R
    from utils import head_sdf
    model, field = driver_scene(tmp_path)
    own = np.asarray(R.mixed_model([5, 40, 64, 65, 130, 1, 17], device="cpu", seed=21).ref_strand_root, np.float64)
    capture = tmp_path / "capture"
    os.makedirs(capture)
    save_head_reconstruction_data_npz(str(capture / "head_reconstruction_data.npz"), own, own)
    shutil.copy(field, capture / head_sdf.FILE)
    common = ["-m", str(model), "-s", str(capture), "--device", "cpu", "--points", "9", "--interpolate"]
    off, _ = export_strands.main(common + ["-o", str(tmp_path / "off")])
    text = capsys.readouterr().out
    assert "Inside the head" in text and "(they are written as they are)" in text
    on, _ = export_strands.main(common + ["-o", str(tmp_path / "on"), "--resolve_head"])
    text = capsys.readouterr().out
    assert "written as they are" not in text and "inside the head before:" in text and str(capture / head_sdf.FILE) in text
    assert on.n_strands == off.n_strands == 14 and not CR.same_bytes(on.points, off.points)


def test_driver_refuses_without_a_field(tmp_path, capsys):
    import export_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    os.makedirs(tmp_path / "capture")
    for extra in ([], ["-s", str(tmp_path / "capture")], ["--head_sdf", str(tmp_path / "nothing.npz")]):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), "--resolve_head"] + extra)
        assert stop.value.code == 2
        err = capsys.readouterr().err
        assert "export_strands.py: --resolve_head" in err and "head_sdf.py" in err
    assert not os.path.exists(tmp_path / "x.hair")
    for bad in (["--head_margin", "-1"], ["--collide_iters", "0"], ["--collide_iters", "33"]):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), "--resolve_head", "--head_sdf", "f.npz"] + bad)
        assert stop.value.code == 2 and "export_strands.py: --" in capsys.readouterr().err


# ---- the entry point's refusals ------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments():
    """Nothing is launched: these run without a GPU (non-null arguments are the addresses of host buffers that are never read)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    buf, buf2 = C.create_string_buffer(64), C.create_string_buffer(64)
    p, p2 = C.addressof(buf), C.addressof(buf2)
    nan, inf = float("nan"), float("inf")

    def call(K=2, P=5, offsets=p, points=p, phi=p, n=(3, 5, 4), o=(0.0, 0.0, 0.0), inv_h=1.0, margin=0.0, skin=0.0, iters=8, out=p2, moved=p,
             unresolved=p):
        status = L.hgs_strand_collide(None, K, offsets, P, points, phi, n[0], n[1], n[2], o[0], o[1], o[2], inv_h, margin, skin, iters, out,
                                      moved, unresolved)
        return status, L.hgs_last_error().decode()

    for kw, words in ((dict(K=-1), "bad sizes"), (dict(P=-1), "bad sizes"), (dict(iters=0), "iters = 0"), (dict(iters=33), "iters = 33"),
                      (dict(margin=-1.0), "margin"), (dict(margin=nan), "margin"), (dict(margin=inf), "margin"), (dict(skin=-1.0), "skin"),
                      (dict(skin=nan), "skin"), (dict(skin=inf), "skin"), (dict(n=(1, 5, 4)), "grid"), (dict(n=(3, 1, 4)), "grid"),
                      (dict(n=(3, 5, 1)), "grid"), (dict(n=(1025, 5, 4)), "grid"), (dict(n=(3, 5, 1025)), "grid"), (dict(inv_h=0.0), "1/h"),
                      (dict(inv_h=nan), "1/h"), (dict(o=(nan, 0.0, 0.0)), "origin"), (dict(offsets=None), "null"), (dict(points=None), "null"),
                      (dict(phi=None), "null"), (dict(out=None), "null"), (dict(moved=None), "null"), (dict(unresolved=None), "null"),
                      (dict(out=p), "alias")):
        status, msg = call(**kw)
        assert status == 1 and "hgs_strand_collide" in msg and words in msg, (kw, msg)
    # nothing to do is not an error, and no pointer is looked at; bad sizes are refused even then
    assert L.hgs_strand_collide(None, 0, None, 0, None, None, 2, 2, 2, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1, None, None, None) == 0
    assert call(K=0, iters=0)[0] == 1 and call(K=0, n=(1, 1, 1))[0] == 1
