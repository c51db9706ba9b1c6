"""The root attachment on the CPU (scene/strand_attach.py numpy path, export_strands.py --attach_roots): the vectorised path against
the loop restatement of the contract (tests/attach_reference.py) bit for bit on the hard cases of tests/attach_cases.py, the bits that
must not change, an analytic head that every strand must reach, step lengths to the rounding of the float32 joints, the driver, and
the C entry points' refusals (which launch nothing)."""
import functools
import os
import re

import numpy as np
import pytest

from tests import attach_cases as AC
from tests import attach_reference as AR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def case_inputs(name):
    c = AC.hard_cases()[name]
    return c, AC.field(c["field"]), (AC.volume(c["volume"]) if c["volume"] else None)


@functools.lru_cache(maxsize=None)
def march_reference(name):
    """The restatement's march of one hard case: (ext, count, reason, landed); computed once, shared with the GPU tests."""
    c, sdf, vol = case_inputs(name)
    return AR.march(c["points"], c["offsets"], sdf, vol, **c["knobs"])


@functools.lru_cache(maxsize=None)
def rejoin_reference(name, M):
    c = AC.hard_cases()[name]
    return AR.rejoin(c["points"], c["attrs"], c["offsets"], *march_reference(name)[:3], M)


@functools.lru_cache(maxsize=None)
def counted_reference():
    """The restatement on the 1000-strand case, its march and its rejoin for every M; strands are independent, so its first K strands
    are the case of K strands."""
    pts, attrs, off = AC.sphere_strands()
    m = AR.march(pts, off, AC.field(AC.COUNTED["field"]), AC.volume(AC.COUNTED["volume"]), **AC.COUNTED["knobs"])
    return m, {M: AR.rejoin(pts, attrs, off, *m[:3], M) for M in AC.MS}


def counted_slice(K, M):
    """The first K strands of counted_reference: (march, rejoin)."""
    m, r = counted_reference()
    out, oat, out_off = r[M]
    return tuple(v[:K] for v in m), (out[:out_off[K]], oat[:out_off[K]], out_off[:K + 1])


def assert_same(got, ref, what, names=("ext", "count", "reason", "landed")):
    assert len(got) == len(ref)
    for name, a, b in zip(names, got, ref):
        assert AR.same_bytes(np.asarray(a), b), (what, name)


REJOINED = ("points", "attrs", "offsets")


def masked(march):
    """A march with the rows of ext from count on zeroed: they are unspecified."""
    ext, count = np.array(march[0], copy=True), march[1]
    ext[np.arange(ext.shape[1])[None, :] >= count[:, None]] = 0.0
    return (ext,) + tuple(march[1:])


def test_the_case_names_are_the_cases():
    assert tuple(AC.hard_cases()) == AC.HARD_NAMES


@pytest.mark.parametrize("name", AC.HARD_NAMES)
def test_numpy_march_matches_the_loop_restatement(name):
    from scene.strand_attach import attach_numpy
    c, sdf, vol = case_inputs(name)
    got = attach_numpy(c["points"], c["offsets"], sdf, vol, **c["knobs"])
    assert_same(got, march_reference(name), name)


@pytest.mark.parametrize("M", AC.MS)
@pytest.mark.parametrize("name", AC.HARD_NAMES)
def test_numpy_rejoin_matches_the_loop_restatement(name, M):
    from scene.strand_attach import rejoin_numpy
    c = AC.hard_cases()[name]
    got = rejoin_numpy(c["points"], c["attrs"], c["offsets"], *march_reference(name)[:3], M)
    assert_same(got, rejoin_reference(name, M), (name, M), REJOINED)
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32 and got[2].dtype == np.int64


@pytest.mark.parametrize("K", AC.KS)
def test_numpy_path_at_every_strand_count(K):
    from scene.strand_attach import attach_numpy, rejoin_numpy
    pts, attrs, off = AC.first_strands(*AC.sphere_strands(), K)
    got = attach_numpy(pts, off, AC.field(AC.COUNTED["field"]), AC.volume(AC.COUNTED["volume"]), **AC.COUNTED["knobs"])
    for M in AC.MS:
        m, r = counted_slice(K, M)
        assert_same(got, m, f"K={K}")
        assert_same(rejoin_numpy(pts, attrs, off, *got[:3], M), r, f"K={K} M={M}", REJOINED)


def test_the_cases_exercise_what_they_are_meant_to():
    """The restatement's own results say that every branch of the contract is taken."""
    R = AR
    _, index = AC.special_strands("sphere9", 0.0, 0.45)
    ext, count, reason, landed = march_reference("special_sphere9_m0.0_None")
    why = {k: int(reason[i]) for k, i in index.items()}
    assert why["empty"] == why["one"] == why["one_nan"] == R.DEGENERATE
    assert why["near_last"] == R.NEAR and why["near_first"] == R.REACHED and count[index["near_first"]] == 1    # lands without a step
    assert why["inside"] == why["centre"] == R.NEAR and landed[index["inside"]] < 0
    for k in ("outside", "at_top", "below", "nan_root", "inf_root", "ninf_root", "huge_root"):
        assert why[k] == R.RANGE and count[index[k]] == 0, k
    for k in ("nan_second", "inf_second", "doubled", "far_last", "away", "sideways", "inward", "two"):
        assert why[k] == R.REACHED, k
    assert why["far_first"] == R.FAR and why["corner"] == R.FAR and why["long"] == R.FAR
    assert np.isinf(landed[reason >= R.DEGENERATE]).all() and np.isfinite(landed[reason <= R.NEAR]).all()
    # without a tangent the march starts straight down the gradient: its first step is radial on a sphere
    i = index["nan_second"]
    first = ext[i, 0] - np.array([1.3, 0.2, 0.1], np.float32).astype(np.float64)
    assert count[i] >= 2 and np.dot(first / np.linalg.norm(first), -np.array([1.3, 0.2, 0.1]) / np.linalg.norm([1.3, 0.2, 0.1])) > 0.99
    # a tangent that points away is clamped to the way down (the field's own gradient: one-sided on a node plane, hence the slack in y)
    j = index["away"]
    assert count[j] >= 2 and ext[j, 0, 0] < 1.4 - 0.2 and abs(ext[j, 0, 1]) < 0.1
    # the volume steers: the same strands take other paths with it, and none where its conf is zero
    plain, zero = march_reference("special_sphere9_m0.0_None"), march_reference("special_sphere9_m0.0_zero_pull4.0")
    swirl = march_reference("special_sphere24_m0.02_swirl_pull0.5")
    assert not AR.same_bytes(swirl[0], march_reference("special_sphere24_m0.0_const_pull0.0_descent0.5")[0]) and plain[2].tolist() == zero[2].tolist()
    assert (march_reference("special_sphere24_m0.02_swirl_pull0.5_min_conf0.2_land_iters1")[2] == R.UNLANDED).sum() >= 1
    assert (march_reference("special_sphere24_m0.0_None_tol0.0_land_iters8_step0.05_descent1.0")[2] == R.UNLANDED).sum() >= 5
    assert march_reference("steps_exact")[2].tolist() == [R.REACHED] and march_reference("steps_one_short")[2].tolist() == [R.STEPS]
    c = AC.hard_cases()["steps_exact"]
    assert march_reference("steps_exact")[1][0] == c["knobs"]["max_steps"] == march_reference("steps_one_short")[1][0] + 1
    assert (march_reference("scene_small_steps")[2] == R.STEPS).sum() > 20 and (march_reference("scene_one_step")[2] == R.STEPS).sum() > 20
    p_count, p_reason = march_reference("plateau")[1:3]
    assert p_reason.tolist() == [R.FLAT] * 4 and p_count[0] == 0 and p_count[1] > 0          # at once, and after marching into the cell
    assert march_reference("flat")[2].tolist() == [R.NEAR, R.REACHED, R.REACHED, R.NEAR]     # (there the flat cells are inside the head)
    t_count, t_reason = march_reference("tiny")[1:3]
    assert t_reason.tolist() == [R.RANGE, R.REACHED, R.RANGE] and t_count[0] >= 1 and t_count[2] == 0   # leaves the cell; rooted outside it
    for name in ("slab", "slab_margin"):
        tally = np.bincount(march_reference(name)[2], minlength=8)
        assert tally[R.REACHED] > 10 and tally[R.RANGE] > 10 and tally[R.NEAR] > 3, (name, tally)
    m, _ = counted_reference()
    assert (m[2] == R.REACHED).sum() > 800 and (m[2] == R.DEGENERATE).sum() > 60 and m[1].max() >= 3


def test_negating_volume_entries_changes_no_bit():
    for a, b in (("scene_swirl", "scene_flip"),
                 ("special_sphere24_m0.02_swirl_pull0.5_min_conf0.2_land_iters1", "special_sphere24_m0.02_flip_pull0.5_min_conf0.2_land_iters1")):
        assert not AR.same_bytes(AC.volume("swirl").dir, AC.volume("flip").dir)
        assert_same(march_reference(a), march_reference(b), (a, b))
        assert march_reference(a)[1].max() >= 5


# ---- the entry point: what must not change, and what must hold --------------------------------------------------------------------------
def as_strands(points, attrs, offsets):
    from scene.strand_export import StrandExport
    K = offsets.shape[0] - 1
    return StrandExport(points, attrs, offsets, np.arange(K, dtype=np.int64) + 3, np.zeros(K))


@pytest.mark.parametrize("name", ("special_sphere9_m0.05_swirl", "scene_swirl", "scene_small_steps", "slab_margin", "tiny"))
def test_bits_that_must_not_change(name):
    """A strand that is already rooted, and one whose march fails, keep every bit in both modes; in ragged mode the original joints of
    a strand that reached keep theirs, behind the new joints, which carry the root's attributes."""
    from scene.strand_attach import REACHED, attach_roots
    from scene.strand_collide import strand_lengths
    c, sdf, vol = case_inputs(name)
    pts, attrs, off = c["points"], c["attrs"], c["offsets"]
    _, count, reason, _ = march_reference(name)
    for M in (0, 7):
        res, rep = attach_roots(as_strands(pts, attrs, off), sdf, vol, points=M, **c["knobs"])
        assert rep["reason"].tolist() == reason.tolist() and np.array_equal(res.strand_ids, np.arange(off.shape[0] - 1) + 3)
        assert rep["attached"] == int((reason == REACHED).sum()) and rep["joints_added"] == int(count[reason == REACHED].sum())
        assert AR.same_bytes(res.length, strand_lengths(res.points, res.offsets))
        for s in range(off.shape[0] - 1):
            a, b, oa, ob = int(off[s]), int(off[s + 1]), int(res.offsets[s]), int(res.offsets[s + 1])
            if reason[s] != REACHED:
                assert AR.same_bytes(res.points[oa:ob], pts[a:b]) and AR.same_bytes(res.attrs[oa:ob], attrs[a:b]), (s, M)
            elif M == 0:
                k = int(count[s])
                assert ob - oa == b - a + k and AR.same_bytes(res.points[oa + k:ob], pts[a:b]) and AR.same_bytes(res.attrs[oa + k:ob], attrs[a:b]), s
                assert AR.same_bytes(res.attrs[oa:oa + k], np.repeat(attrs[a:a + 1], k, axis=0)), s
            else:
                assert ob - oa == M and AR.same_bytes(res.points[ob - 1], pts[b - 1]) and AR.same_bytes(res.attrs[ob - 1], attrs[b - 1]), s
                assert AR.same_bytes(res.attrs[oa], attrs[a]) and not AR.same_bytes(res.points[oa], pts[a]), s
    assert (reason == REACHED).sum() >= 1 and (reason != REACHED).sum() >= 1


def segment_bound(a, b):
    """What the rounding of two float32 endpoints allows a segment's length to change by: every coordinate of an endpoint is off by at
    most half a unit in its last place, so the segment's vector by at most the sum of the two per coordinate."""
    ha, hb = (0.5 * np.spacing(np.abs(v)).astype(np.float64) for v in (a, b))
    return np.sqrt(((ha + hb) ** 2).sum(axis=1))


@functools.lru_cache(maxsize=None)
def landing_result(grid, margin, pull):
    from scene.strand_attach import attach_numpy
    pts, _, off = AC.landing_strands()
    return attach_numpy(pts, off, AC.field(f"sphere{grid}"), None, margin=margin, pull=pull)


@pytest.mark.parametrize("pull", AC.LANDING_PULLS)
@pytest.mark.parametrize("margin", AC.LANDING_MARGINS)
@pytest.mark.parametrize("grid", AC.LANDING_GRIDS)
def test_every_strand_reaches_the_analytic_head(grid, margin, pull):
    """Roots at radius 1.03 to 1.6 around the unit sphere, step half a spacing, descent 0.25, 4 landing steps: every strand is REACHED
    and lands within tol; every marched segment has the step's length up to the float32 rounding of the joints (and a relative 1e-12
    for the float64 arithmetic that placed them: a few thousand times its rounding)."""
    from scene.strand_attach import REACHED, default_tol, rejoin_numpy
    pts, attrs, off = AC.landing_strands()
    sdf = AC.field(f"sphere{grid}")
    ext, count, reason, landed = landing_result(grid, margin, pull)
    m, tol, step = np.float64(np.float32(margin)), np.float64(default_tol(sdf)), 0.5 * sdf.spacing
    err = np.abs(landed.astype(np.float64) - m)
    print(f"grid {grid} margin {margin} pull {pull}: reached {(reason == REACHED).sum()} of {reason.shape[0]}, joints added at most {count.max()}, "
          f"largest |d - margin| {err.max():.3g} (tol {tol:.3g})")
    assert reason.shape[0] == 300 and (reason == REACHED).all()
    assert (err <= tol).all() and count.min() >= 1
    out, _, out_off = rejoin_numpy(pts, attrs, off, ext, count, reason, 0)
    worst = 0.0
    for s in range(300):
        k = int(count[s])
        if k < 2:
            continue
        run = out[out_off[s] + 1:out_off[s] + k + 1]                              # x_k .. x_1, p_0: the marched segments (not the landing's)
        a, b = run[:-1], run[1:]
        got = np.linalg.norm(b.astype(np.float64) - a.astype(np.float64), axis=1)
        bound = segment_bound(a, b) + 1e-12 * step
        worst = max(worst, float((np.abs(got - step) / step).max()))
        assert (np.abs(got - step) <= bound).all(), (s, float((np.abs(got - step) - bound).max()))
    print(f"largest relative deviation of a marched segment from the step: {worst:.3g}")
    # the landed point as it is written (rounded to float32) is still where the field says it is, to the rounding of its coordinates
    from utils.head_sdf import trilinear
    ok, d, _, _, _ = trilinear(out[out_off[:-1]], sdf)
    assert ok.all() and (np.abs(d.astype(np.float64) - m) <= tol + 4.0 * np.spacing(np.float32(2.0))).all()


def test_the_restatement_alone_reaches_the_analytic_head():
    """One configuration by the loop restatement itself, with a volume as well: every strand REACHED."""
    pts, _, off = AC.landing_strands()
    for vol in (None, AC.volume("swirl")):
        _, count, reason, landed = AR.march(pts, off, AC.field("sphere24"), vol, margin=0.02, pull=0.5)
        assert (reason == AR.REACHED).all() and count.max() <= 32
        assert (np.abs(landed.astype(np.float64) - np.float64(np.float32(0.02))) <= np.float64(np.float32(1e-3 * AC.field("sphere24").spacing))).all()


def test_attach_roots_batches_reports_and_tests_the_scalp():
    from scene import strand_attach as SA
    c, sdf, vol = case_inputs("scene_swirl")
    strands = as_strands(c["points"], c["attrs"], c["offsets"])
    whole, rep = SA.attach_roots(strands, sdf, vol, points=5, **c["knobs"])
    parts, rep2 = SA.attach_roots(strands, sdf, vol, points=5, budget=24 * 257 * 7, **c["knobs"])       # 7 strands a batch
    for a, b in zip(whole, parts):
        assert AR.same_bytes(a, b)
    assert {k: v for k, v in rep.items() if k != "reason"} == {k: v for k, v in rep2.items() if k != "reason"}
    assert rep["strands"] == 120 and rep["attached"] + rep["near"] + sum(rep["failed"].values()) == 120 and rep["failed"] == {"degenerate": 23}
    assert 0.5 < rep["gap_max"] < 0.7 and 0.0 < rep["gap_mean"] < rep["gap_max"] and rep["landed_error"] <= float(SA.default_tol(sdf))
    # the scalp: the landed roots of the upper half only; the strands that landed below are restored bit for bit
    ext, count, reason, _ = march_reference("scene_swirl")
    hit = np.nonzero(reason == SA.REACHED)[0]
    landed = ext[hit, count[hit] - 1]
    scalp = landed[landed[:, 2] > 0.0]
    res, rep3 = SA.attach_roots(strands, sdf, vol, points=0, scalp_points=scalp, scalp_distance=1e-3, **c["knobs"])
    off_scalp = hit[landed[:, 2] <= 0.0]
    assert 10 < off_scalp.shape[0] < hit.shape[0] - 10 and rep3["failed"]["off_scalp"] == off_scalp.shape[0]
    assert np.array_equal(np.nonzero(rep3["reason"] == SA.OFF_SCALP)[0], off_scalp) and rep3["attached"] == hit.shape[0] - off_scalp.shape[0]
    for s in off_scalp[:5]:
        assert AR.same_bytes(res.points[res.offsets[s]:res.offsets[s + 1]], c["points"][c["offsets"][s]:c["offsets"][s + 1]])
    kept = SA.select_strands(res, rep3["reason"] <= SA.NEAR)
    assert kept.n_strands == rep3["attached"] + rep3["near"] and kept.offsets[-1] == kept.points.shape[0] == kept.attrs.shape[0]
    first = int(np.nonzero(rep3["reason"] <= SA.NEAR)[0][0])
    assert AR.same_bytes(kept.points[:kept.offsets[1]], res.points[res.offsets[first]:res.offsets[first + 1]]) and kept.strand_ids[0] == first + 3


def test_arguments_are_checked():
    from scene.strand_attach import attach_numpy, attach_roots, rejoin_numpy
    from utils.head_sdf import HeadSDF
    c, sdf, _ = case_inputs("tiny")
    pts, attrs, off = c["points"], c["attrs"], c["offsets"]
    nan, inf = np.nan, np.inf
    for kw, words in ((dict(margin=-0.1), "margin"), (dict(margin=nan), "margin"), (dict(margin=inf), "margin"), (dict(tol=-1.0), "tol"), (dict(tol=nan), "tol"),
                      (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=inf), "step"), (dict(step=nan), "step"), (dict(max_steps=0), "max_steps"),
                      (dict(max_steps=1025), "max_steps"), (dict(max_steps=2.5), "max_steps"), (dict(land_iters=0), "land_iters"), (dict(land_iters=9), "land_iters"),
                      (dict(pull=-1.0), "pull"), (dict(pull=inf), "pull"), (dict(pull=nan), "pull"), (dict(descent=0.0), "descent"), (dict(descent=1.5), "descent"),
                      (dict(descent=nan), "descent"), (dict(max_distance=-1.0), "max_distance"), (dict(max_distance=nan), "max_distance"),
                      (dict(min_conf=nan), "min_conf"), (dict(min_conf=inf), "min_conf")):
        with pytest.raises(ValueError, match=words):
            attach_numpy(pts, off, sdf, **kw)
    assert attach_numpy(pts, off, sdf, max_distance=inf, max_steps=1024, land_iters=8, descent=1.0, pull=0.0)[2].shape == (3,)
    for bad in (off[1:], off[:-1], off[::-1].copy(), off.astype(np.float64)):
        with pytest.raises(ValueError, match="offsets"):
            attach_numpy(pts, bad, sdf)
    with pytest.raises(ValueError, match="points"):
        attach_numpy(pts.reshape(-1), off, sdf)
    with pytest.raises(ValueError, match="at least 2"):
        attach_numpy(pts, off, HeadSDF(np.zeros(3), 1.0, (3, 1, 2), np.zeros((2, 1, 3), np.float32)))
    ext, count, reason, _ = march_reference("tiny")
    for kw, words in ((dict(M=1), "M = 1"), (dict(M=-2), "M = -2"), (dict(ext=ext[:2]), "ext"), (dict(ext=ext.astype(np.float32)), "ext"),
                      (dict(count=count[:2]), "count"), (dict(count=count.astype(np.int64)), "count"), (dict(reason=reason[:1]), "reason"),
                      (dict(count=count + 1000), "count outside"), (dict(attrs=attrs[:-1]), "attrs"), (dict(attrs=np.zeros((pts.shape[0], 65), np.float32)), "attrs")):
        args = dict(points=pts, attrs=attrs, offsets=off, ext=ext, count=count, reason=reason, M=0)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            rejoin_numpy(**args)
    strands = as_strands(pts, attrs, off)
    for kw, words in ((dict(device="cpu"), "device"), (dict(points=1), "points"), (dict(scalp_distance=1.0), "scalp"), (dict(scalp_points=np.zeros((0, 3)), scalp_distance=1.0), "scalp"),
                      (dict(scalp_points=np.zeros((2, 3)), scalp_distance=-1.0), "scalp"), (dict(pull=-1.0), "pull")):
        with pytest.raises(ValueError, match=words):
            attach_roots(strands, sdf, **kw)


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_library_agree():
    import ctypes as C
    import hgs_runtime as rt
    assert rt.ABI_VERSION == 15
    header = open(os.path.join(ROOT, "include", "hgs.h")).read()
    assert int(re.search(r"#define\s+HGS_ABI_VERSION\s+(\d+)", header).group(1)) == 15
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kinds = {"void*": C.c_void_p, "int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong}
    L = rt.lib()
    assert L.hgs_abi_version() == 15
    for name in ("hgs_root_attach", "hgs_strand_rejoin"):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", plain, re.S)
        assert decl is not None, name
        want = []
        for arg in decl.group(1).split(","):
            kind = re.sub(r"\bconst\b", "", arg).strip().rsplit(None, 1)[0].strip()
            want.append(C.c_void_p if kind.endswith("*") else kinds[kind])
        res, args = rt.SIGNATURES[name]
        assert res is C.c_int and args == want, (name, args, want)
        assert hasattr(L, name)


def test_entry_points_refuse_bad_arguments():
    """Nothing is launched: these run without a GPU (non-null arguments are the addresses of host buffers that are never read)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    bufs = [C.create_string_buffer(64) for _ in range(12)]
    b = [C.addressof(v) for v in bufs]
    nan, inf = float("nan"), float("inf")

    def attach(K=2, P=5, offsets=b[0], points=b[1], phi=b[2], n=(3, 5, 4), o=(0.0, 0.0, 0.0), inv_h=1.0, vdir=b[3], vconf=b[4], vn=(3, 3, 3),
               vo=(0.0, 0.0, 0.0), vh=0.5, min_conf=0.5, margin=0.0, tol=1e-3, step=0.1, max_steps=8, land_iters=4, pull=1.0, descent=0.25,
               max_distance=inf, ext=b[5], count=b[6], reason=b[7], landed=b[8]):
        status = L.hgs_root_attach(None, K, offsets, P, points, phi, n[0], n[1], n[2], o[0], o[1], o[2], inv_h, vdir, vconf, vn[0], vn[1], vn[2],
                                   vo[0], vo[1], vo[2], vh, min_conf, margin, tol, step, max_steps, land_iters, pull, descent, max_distance, ext,
                                   count, reason, landed)
        return status, L.hgs_last_error().decode()

    for kw, words in ((dict(K=-1), "bad sizes"), (dict(P=-1), "bad sizes"), (dict(max_steps=0), "max_steps = 0"), (dict(max_steps=1025), "max_steps = 1025"),
                      (dict(land_iters=0), "land_iters = 0"), (dict(land_iters=9), "land_iters = 9"), (dict(margin=-1.0), "margin"), (dict(margin=nan), "margin"),
                      (dict(margin=inf), "margin"), (dict(tol=-1.0), "tol"), (dict(tol=nan), "tol"), (dict(step=0.0), "step"), (dict(step=nan), "step"),
                      (dict(step=inf), "step"), (dict(pull=-1.0), "pull"), (dict(pull=inf), "pull"), (dict(descent=0.0), "descent"), (dict(descent=1.5), "descent"),
                      (dict(descent=nan), "descent"), (dict(max_distance=-1.0), "max_distance"), (dict(max_distance=nan), "max_distance"),
                      (dict(n=(1, 5, 4)), "head field"), (dict(n=(3, 5, 1025)), "head field"), (dict(inv_h=0.0), "1/h"), (dict(inv_h=nan), "1/h"),
                      (dict(o=(nan, 0.0, 0.0)), "origin"), (dict(vconf=None), "come together"), (dict(vdir=None), "come together"),
                      (dict(vn=(1, 3, 3)), "volume"), (dict(vn=(3, 3, 1025)), "volume"), (dict(vn=(1024, 1024, 1024)), "volume"), (dict(vh=0.0), "spacing"),
                      (dict(vh=nan), "spacing"), (dict(vo=(0.0, inf, 0.0)), "spacing"), (dict(min_conf=nan), "min_conf"), (dict(offsets=None), "null"),
                      (dict(points=None), "null"), (dict(phi=None), "null"), (dict(ext=None), "null"), (dict(count=None), "null"), (dict(reason=None), "null"),
                      (dict(landed=None), "null"), (dict(ext=b[1]), "alias"), (dict(ext=b[2]), "alias"), (dict(ext=b[3]), "alias"), (dict(reason=b[6]), "alias"),
                      (dict(landed=b[1]), "alias")):
        status, msg = attach(**kw)
        assert status == 1 and "hgs_root_attach" in msg and words in msg, (kw, msg)
    # nothing to do is not an error, and no pointer is looked at; bad sizes are refused even then; the volume may be absent
    assert attach(K=0, P=0, offsets=None, points=None, phi=None, vdir=None, vconf=None, ext=None, count=None, reason=None, landed=None)[0] == 0
    assert attach(K=0, max_steps=0)[0] == 1 and attach(K=0, n=(1, 1, 1))[0] == 1 and attach(K=0, vdir=None, vconf=None, vn=(0, 0, 0), vh=nan)[0] == 0

    def rejoin(K=2, P=5, offsets=b[0], points=b[1], attrs=b[2], C_=3, ext=b[3], rows=9, count=b[4], reason=b[5], M=0, out_off=b[6], n_out=7, out=b[7],
               oat=b[8]):
        status = L.hgs_strand_rejoin(None, K, offsets, P, points, attrs, C_, ext, rows, count, reason, M, out_off, n_out, out, oat)
        return status, L.hgs_last_error().decode()

    for kw, words in ((dict(K=-1), "bad sizes"), (dict(P=-1), "bad sizes"), (dict(n_out=-1), "bad sizes"), (dict(C_=-1), "channels"), (dict(C_=65), "channels"),
                      (dict(M=1), "M = 1"), (dict(M=-3), "M = -3"), (dict(rows=1), "ext_rows"), (dict(rows=1026), "ext_rows"), (dict(offsets=None), "null"),
                      (dict(points=None), "null"), (dict(attrs=None), "null"), (dict(ext=None), "null"), (dict(count=None), "null"), (dict(reason=None), "null"),
                      (dict(out_off=None), "null"), (dict(out=None), "null"), (dict(oat=None), "null"), (dict(out=b[1]), "alias"), (dict(out=b[2]), "alias"),
                      (dict(out=b[3]), "alias"), (dict(oat=b[2]), "alias"), (dict(oat=b[1]), "alias"), (dict(oat=b[7]), "alias")):
        status, msg = rejoin(**kw)
        assert status == 1 and "hgs_strand_rejoin" in msg and words in msg, (kw, msg)
    assert rejoin(K=0, P=0, offsets=None, points=None, attrs=None, ext=None, count=None, reason=None, out_off=None, n_out=0, out=None, oat=None)[0] == 0
    assert rejoin(K=0, M=1)[0] == 1 and rejoin(K=0, rows=0)[0] == 1


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
def driver_volume(tmp_path, sdf):
    """A direction volume file over the field's box: one direction everywhere."""
    from utils.trace import Field, save_field
    g = 6
    h = (max(sdf.shape) - 1) * sdf.spacing / (g - 1)
    d = np.broadcast_to(np.array([0.6, 0.0, 0.8]), (g, g, g, 3)).copy()
    path = tmp_path / "volume.npz"
    save_field(str(path), Field(sdf.origin, h, (g, g, g), d, np.ones((g, g, g))))
    return path


def test_driver_attaches_roots(tmp_path, capsys):
    import export_strands
    from data import strand_files as F
    from scene import strand_attach as SA
    from scene.strand_export import resample_strands
    from tests.test_collide_cpu import driver_scene
    from utils import head_sdf
    from utils.system import model_ply
    from utils.trace import load_field
    model, field = driver_scene(tmp_path)
    sdf = head_sdf.load_sdf(str(field))
    volume = driver_volume(tmp_path, sdf)
    common = ["-m", str(model), "--device", "cpu", "--format", "hair", "--format", "usc"]
    for points in ("9", "0"):                                                     # resampled, and the joints as they are (ragged)
        capsys.readouterr()
        plain, pp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"plain{points}")])
        assert "Attached to the head" not in capsys.readouterr().out
        # without the flag the files are the writers' bytes of the resampled strands: what they were before there was a flag
        m = export_strands.load_strand_model(model_ply(str(model)), None, device="cpu")
        direct = resample_strands(m, points=int(points), min_segments=1, min_length=0.0, max_root_distance=None, device=None)
        F.write_strands_cy(str(tmp_path / "direct.hair"), direct)
        F.write_strands_usc(str(tmp_path / "direct.data"), direct)
        assert open(pp["hair"], "rb").read() == open(tmp_path / "direct.hair", "rb").read()
        assert open(pp["usc"], "rb").read() == open(tmp_path / "direct.data", "rb").read()
        for tag, extra, kw in (("plain", [], {}), ("steered", ["--attach_field", str(volume), "--attach_margin", "0.001", "--attach_pull", "0.5", "--attach_step",
                                                              str(0.3 * sdf.spacing), "--attach_max_steps", "300", "--attach_descent", "0.3", "--attach_min_conf", "0.25"],
                                                   dict(field=load_field(str(volume)), margin=0.001, pull=0.5, step=0.3 * sdf.spacing, max_steps=300, descent=0.3,
                                                        min_conf=0.25))):
            res, rp = export_strands.main(common + ["--points", points, "-o", str(tmp_path / f"att{points}{tag}"), "--attach_roots", "--head_sdf", str(field)] + extra)
            text = capsys.readouterr().out
            want, rep = SA.attach_roots(plain, sdf, points=int(points), **kw)
            assert rep["attached"] >= 3 and rep["near"] >= 1 and rep["joints_added"] > rep["attached"], rep
            for a, b in zip(res, want):
                assert AR.same_bytes(a, b), (points, tag)
            assert f"{rep['attached']} of {rep['strands']} strands attached, {rep['near']} already rooted, {sum(rep['failed'].values())} failed" in text
            assert f"{rep['joints_added']} joints added" in text and "root gap before: largest" in text and "largest |d - margin| of the landed roots" in text
            assert ("steered by" in text) == (tag == "steered")
            if points == "9":
                assert np.array_equal(res.offsets, plain.offsets) and not AR.same_bytes(res.points, plain.points)
            else:
                assert res.points.shape[0] == plain.points.shape[0] + rep["joints_added"]
            F.write_strands_cy(str(tmp_path / "want.hair"), want)
            assert open(rp["hair"], "rb").read() == open(tmp_path / "want.hair", "rb").read() != open(pp["hair"], "rb").read()
    # strands too far from the head stay; dropping the failed ones; the scalp test against the model's own strand roots
    far, _ = export_strands.main(common + ["--points", "9", "-o", str(tmp_path / "far"), "--attach_roots", "--head_sdf", str(field), "--attach_max_distance", "0"])
    text = capsys.readouterr().out
    assert "0 of 7 strands attached" in text and "far " in text and ", 0 dropped" in text and far.n_strands == 7
    drop, _ = export_strands.main(common + ["--points", "9", "-o", str(tmp_path / "drop"), "--attach_roots", "--head_sdf", str(field), "--attach_max_distance", "0",
                                            "--drop_unattached"])
    text = capsys.readouterr().out
    assert 0 < drop.n_strands < 7 and f"{7 - drop.n_strands} dropped" in text and drop.offsets[-1] == drop.points.shape[0] == 9 * drop.n_strands
    off, _ = export_strands.main(common + ["--points", "9", "-o", str(tmp_path / "scalp"), "--attach_roots", "--head_sdf", str(field), "--attach_scalp_distance", "1e-9"])
    text = capsys.readouterr().out
    p9, _ = export_strands.main(common + ["--points", "9", "-o", str(tmp_path / "p9")])
    assert "0 of 7 strands attached" in text and "off_scalp " in text and AR.same_bytes(off.points, p9.points) and AR.same_bytes(off.attrs, p9.attrs)
    capsys.readouterr()
    near, _ = export_strands.main(common + ["--points", "9", "-o", str(tmp_path / "scalp2"), "--attach_roots", "--head_sdf", str(field), "--attach_scalp_distance", "1e9"])
    assert "off_scalp" not in capsys.readouterr().out and AR.same_bytes(near.points, SA.attach_roots(p9, sdf, points=9)[0].points)


def test_driver_combines_with_interpolate_and_resolve_head(tmp_path, capsys):
    """Guides are rooted before they are blended, and the new joints are pushed out with the rest: the three steps in the driver's order
    give what the three entry points give one after the other."""
    import export_strands
    from scene import strand_attach as SA
    from scene.strand_collide import resolve_head
    from tests.test_collide_cpu import driver_scene
    from utils import head_sdf
    model, field = driver_scene(tmp_path)
    sdf = head_sdf.load_sdf(str(field))
    common = ["-m", str(model), "--device", "cpu", "--points", "9"]
    plain, _ = export_strands.main(common + ["-o", str(tmp_path / "plain")])
    both, _ = export_strands.main(common + ["-o", str(tmp_path / "both"), "--attach_roots", "--resolve_head", "--head_sdf", str(field), "--head_margin", "0.001"])
    text = capsys.readouterr().out
    assert text.index("Attached to the head") < text.index("Resolved against the head")
    rooted, _ = SA.attach_roots(plain, sdf, points=9)
    want, _ = resolve_head(rooted, sdf, margin=0.001)
    assert AR.same_bytes(both.points, want.points) and AR.same_bytes(both.length, want.length)
    groom, _ = export_strands.main(common + ["-o", str(tmp_path / "groom"), "--attach_roots", "--interpolate", "--resolve_head", "--head_sdf", str(field)])
    text = capsys.readouterr().out
    assert text.index("Attached to the head") < text.index("Interpolated:") < text.index("Resolved against the head")
    loose, _ = export_strands.main(common + ["-o", str(tmp_path / "loose"), "--interpolate", "--resolve_head", "--head_sdf", str(field)])
    assert groom.n_strands == loose.n_strands > 7 and AR.same_bytes(groom.offsets, loose.offsets) and not AR.same_bytes(groom.points, loose.points)


def test_driver_refuses_without_a_field_and_bad_values(tmp_path, capsys):
    import export_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    os.makedirs(tmp_path / "capture")
    for extra in ([], ["-s", str(tmp_path / "capture")], ["--head_sdf", str(tmp_path / "nothing.npz")]):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), "--attach_roots"] + extra)
        assert stop.value.code == 2
        err = capsys.readouterr().err
        assert "export_strands.py: --attach_roots" in err and "head_sdf.py" in err
    assert not os.path.exists(tmp_path / "x.hair")
    for bad in (["--attach_margin", "-1"], ["--attach_margin", "nan"], ["--attach_step", "0"], ["--attach_max_steps", "0"], ["--attach_max_steps", "1025"],
                ["--attach_pull", "-1"], ["--attach_descent", "0"], ["--attach_descent", "1.5"], ["--attach_max_distance", "-1"], ["--attach_min_conf", "nan"],
                ["--attach_scalp_distance", "-1"], ["--attach_field", str(tmp_path / "nothing.npz")]):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), "--attach_roots", "--head_sdf", "f.npz"] + bad)
        assert stop.value.code == 2 and f"export_strands.py: {bad[0]}" in capsys.readouterr().err, bad
    # without --attach_roots its options are ignored, bad values included
    out, _ = export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "y"), "--attach_max_steps", "0", "--attach_margin", "-1", "--drop_unattached"])
    assert out.n_strands == 7
