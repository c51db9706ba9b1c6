"""The guide selection on the CPU (scene/strand_guides.py numpy path, export_strands.py --select_guides): the vectorised path against
the loop restatement of the contract (tests/guides_reference.py) bit for bit on the cases of tests/guides_cases.py, properties checked
independently of both, the refusals, the entry point's strands and binding, the C entry points' refusals (which launch nothing) and
the driver."""
import functools
import os
import re

import numpy as np
import pytest

from tests import guides_cases as GC
from tests import guides_reference as GR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of one case; computed once, shared with the GPU tests."""
    pts, off, k, samples, iters = GC.cases()[name]
    return GR.guides(pts, off, k, samples, iters)


@functools.lru_cache(maxsize=None)
def numpy_result(name):
    from scene.strand_guides import guides_numpy
    return guides_numpy(*GC.cases()[name])


def assert_same(got, ref, what):
    for name, a, b in zip(GC.FIELDS, got, ref):
        if name in ("iterations", "converged"):
            assert a == b and type(a) is type(b), (what, name, a, b)
        else:
            assert GR.same_bytes(a, b), (what, name)


def brute_labels(x, cent):
    """(label, d2) of float64 features [n, S, 3] against centroids [K, S, 3]: every d2 on its own, the argmin by (d2, k) by sorting."""
    n, K, S = x.shape[0], cent.shape[0], x.shape[1]
    d = np.zeros((n, K))
    for s in range(S):
        t = x[:, None, s, :] - cent[None, :, s, :]
        d = d + ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])
    lab = np.array([sorted(range(K), key=lambda k: (d[i, k], k))[0] for i in range(n)], np.int64)
    return lab, d[np.arange(n), lab]


def features_of(name):
    from scene.strand_guides import sample_joints
    pts, off, k, samples, iters = GC.cases()[name]
    N = off.shape[0] - 1
    M = int(off[1] - off[0])
    S = min(samples, M)
    return pts.reshape(N, M, 3)[:, sample_joints(M, S)].astype(np.float64), S


def test_the_case_names_are_the_cases():
    assert tuple(GC.cases()) == GC.NAMES


@pytest.mark.parametrize("name", GC.NAMES)
def test_numpy_path_matches_the_loop_restatement(name):
    got = numpy_result(name)
    assert_same(got, reference(name), name)
    assert got.labels.dtype == np.int32 and got.dist2.dtype == np.float64 and got.guide.dtype == np.int64 and got.count.dtype == np.int32
    assert got.status.dtype == np.int32


def test_the_cases_exercise_what_they_are_meant_to():
    """The restatement's own results say that every branch of the contract is taken."""
    R = {n: dict(zip(GC.FIELDS, reference(n))) for n in GC.NAMES}
    N = lambda n: GC.cases()[n][1].shape[0] - 1
    assert sorted({N(n) for n in GC.NAMES} & {1, 63, 64, 65, 257, 1000}) == [1, 63, 64, 65, 257, 1000]
    assert {int(GC.cases()[n][1][1]) for n in GC.NAMES} >= {2, 3, 17, 100}
    assert {R[n]["centroids"].shape[1] for n in GC.NAMES} >= {2, 3, 16, 17, 64}
    assert {R[n]["centroids"].shape[0] for n in GC.NAMES} >= {0, 1, 2, 9, 17, 65, 255, 256, 257}
    # k >= N: every eligible strand is its own cluster, every dist2 is 0, guide[k] = E[k]
    for n in ("n257_m2_k257", "k_over_n"):
        r = R[n]
        assert np.array_equal(r["guide"], np.arange(N(n))) and np.array_equal(r["labels"], np.arange(N(n))) and not r["dist2"].any()
        assert r["converged"] and r["iterations"] == 2 and (r["count"] == 1).all()
    # exact duplicates: equal d2, the smaller k and the smaller i win
    r = R["duplicates"]
    assert r["labels"][0] == r["labels"][1] == r["labels"][4] and r["labels"][2] == r["labels"][3] and r["guide"][r["labels"][0]] == 0
    assert r["guide"][r["labels"][2]] == 2 and r["dist2"][0] == r["dist2"][1] == 0.0
    r = R["duplicate_seeds"]
    # (the first assignment gives all eight to cluster 0; once its centroid has moved, the four X tie on the three seeds and take 1)
    assert r["guide"].tolist()[1:] == [1, -1, -1] and r["guide"][0] in (0, 2, 4, 6) and r["count"].tolist() == [4, 4, 0, 0] and r["labels"].tolist() == [0, 1] * 4
    x, _ = features_of("duplicate_seeds")
    assert all(GR.same_bytes(r["centroids"][k], x[1]) for k in (2, 3))             # an empty cluster keeps its centroid
    r = R["nonfinite_unsampled"]
    assert r["status"].tolist() == [1 if i in (3, 7, 12) else 0 for i in range(20)] and r["labels"][3] == r["labels"][7] == -1
    assert np.isinf(r["dist2"][[3, 7, 12]]).all() and np.isfinite(np.delete(r["dist2"], [3, 7, 12])).all() and r["count"].sum() == 17
    x, _ = features_of("nonfinite_unsampled")
    assert np.isfinite(x[[3, 7]]).all() and not np.isfinite(x[12]).all()           # two of the three are bad in a point that is not sampled
    r = R["all_nonfinite"]
    assert r["guide"].shape == (0,) and r["count"].shape == (0,) and (r["labels"] == -1).all() and r["iterations"] == 0 and not r["converged"]
    r = R["near_max"]
    pts = GC.cases()["near_max"][0]
    assert np.isfinite(pts).all() and np.abs(pts).max() > 2.0 ** 124 and np.isfinite(r["dist2"]).all() and r["dist2"].max() > 2.0 ** 250
    r = R["clumps_known"]
    assert np.array_equal(r["labels"], np.repeat(np.arange(4), 16)) and r["converged"] and r["iterations"] < 10
    assert R["iters1"]["iterations"] == 1 and not R["iters1"]["converged"]
    assert R["not_converged"]["iterations"] == 2 and not R["not_converged"]["converged"]
    assert R["n63_m3_k2"]["converged"] and 2 < R["n63_m3_k2"]["iterations"] < 10


@pytest.mark.parametrize("name", GC.NAMES)
def test_labels_are_the_brute_force_argmin_and_guides_are_members(name):
    res = numpy_result(name)
    K = res.guide.shape[0]
    if K == 0:
        return
    x, S = features_of(name)
    E = np.nonzero(res.status == 0)[0]
    lab, d2 = brute_labels(x[E], res.centroids)
    assert np.array_equal(res.labels[E], lab) and GR.same_bytes(res.dist2[E], d2)
    assert np.array_equal(res.count, np.bincount(lab, minlength=K)) and res.count.sum() == E.shape[0]
    for k in range(K):
        members = E[lab == k]
        if members.shape[0] == 0:
            assert res.guide[k] == -1
        else:
            assert res.guide[k] in members
            assert (res.dist2[res.guide[k]], res.guide[k]) == min((res.dist2[i], i) for i in members)


@pytest.mark.parametrize("name", ("n63_m3_k2", "n1000_m3_k2", "not_converged", "clumps_known", "n65_m17_s64_k17"))
def test_total_distance_does_not_increase(name):
    """Lloyd's: an assignment against updated centroids cannot have a larger total than the one before, up to the rounding of the sums
    (relative 1e-12 is orders above n * 2^-53)."""
    from scene.strand_guides import guides_numpy
    pts, off, k, samples, _ = GC.cases()[name]
    totals = []
    for iters in range(1, 7):
        res = guides_numpy(pts, off, k, samples, iters)
        totals.append(float(res.dist2[res.status == 0].sum()))
        if iters == 1:
            assert GR.same_bytes(res.first_dist2, res.dist2)
    print(name, totals)
    assert all(b <= a * (1.0 + 1e-12) for a, b in zip(totals, totals[1:])) and totals[-1] < totals[0]


@pytest.mark.parametrize("name", ("n129_m17_k65", "n257_m2_k256", "n1000_m3_k2", "nonfinite_unsampled"))
def test_the_chunk_budget_does_not_change_the_result(name):
    from scene.strand_guides import guides_numpy
    for budget in (1, 300, 4097):
        assert_same(guides_numpy(*GC.cases()[name], budget=budget), numpy_result(name), (name, budget))


def test_parameters_and_ragged_strands_are_refused():
    from scene.strand_guides import check_parameters, guides_numpy, select_guides, strand_points
    for params, words in GC.REFUSED:
        with pytest.raises(ValueError, match=words):
            check_parameters(*params)
    assert check_parameters(5) == (5, 16, 10) and check_parameters(np.int64(65536), 64, 256) == (65536, 64, 256)
    for pts, off in (GC.ragged(), GC.one_point()):
        with pytest.raises(ValueError, match="same number M >= 2 of points"):
            strand_points(off)
        with pytest.raises(ValueError, match="same number M >= 2 of points"):
            guides_numpy(pts, off, 2)
        with pytest.raises(ValueError, match="same number M >= 2 of points"):
            select_guides(GC.as_export(pts, off), 2)
    pts, off = GC.cases()["n63_m3_k2"][:2]
    with pytest.raises(ValueError, match="offsets"):
        guides_numpy(pts, off[:-1], 2)
    with pytest.raises(ValueError, match="points"):
        guides_numpy(pts.reshape(-1), off, 2)
    with pytest.raises(ValueError, match="device"):
        select_guides(GC.as_export(pts, off), 2, device="cpu")
    empty = guides_numpy(np.zeros((0, 3), np.float32), np.zeros(1, np.int64), 3)
    assert empty.labels.shape == (0,) and empty.guide.shape == (0,) and empty.iterations == 0


@pytest.mark.parametrize("name", ("n63_m3_k2", "duplicate_seeds", "nonfinite_unsampled", "all_nonfinite", "n65_m100_s64_k9"))
def test_select_guides_keeps_the_guides_bits_and_binds_consistently(name):
    from scene.strand_guides import select_guides
    pts, off, k, samples, iters = GC.cases()[name]
    strands = GC.as_export(pts, off)
    guides, binding, rep = select_guides(strands, k, samples, iters)
    res = numpy_result(name)
    N, M = off.shape[0] - 1, int(off[1] - off[0])
    S = min(samples, M)
    g = binding["guide_strand"]
    G = g.shape[0]
    assert g.dtype == np.int64 and binding["strand_guide"].dtype == np.int32 and binding["strand_distance"].dtype == np.float64
    assert binding["cluster_size"].dtype == np.int32 and set(binding) == {"guide_strand", "strand_guide", "strand_distance", "cluster_size"}
    assert np.array_equal(g, res.guide[res.guide >= 0]) and guides.n_strands == G and np.array_equal(guides.offsets, np.arange(G + 1) * M)
    for q, i in enumerate(g):
        assert GR.same_bytes(guides.points[q * M:(q + 1) * M], pts[off[i]:off[i + 1]])
        assert GR.same_bytes(guides.attrs[q * M:(q + 1) * M], strands.attrs[off[i]:off[i + 1]])
    assert np.array_equal(guides.strand_ids, strands.strand_ids[g]) and GR.same_bytes(guides.length, strands.length[g])
    sg = binding["strand_guide"]
    ok = res.status == 0
    assert (sg[~ok] == -1).all() and (sg[ok] >= 0).all() and (sg[ok] < G).all()
    assert np.array_equal(sg[g], np.arange(G))                                     # a guide follows itself
    assert np.array_equal(np.bincount(sg[ok], minlength=G), binding["cluster_size"]) and binding["cluster_size"].sum() == ok.sum()
    assert np.array_equal(res.labels[ok], np.nonzero(res.guide >= 0)[0][sg[ok]])
    assert GR.same_bytes(binding["strand_distance"], np.sqrt(res.dist2 / float(S)))
    assert set(rep) == {"strands", "eligible", "nonfinite", "clusters_asked", "clusters_made", "clusters_empty", "iterations", "converged",
                        "size_min", "size_mean", "size_max", "distance_mean", "distance_max", "total_first", "total_last"}
    assert (rep["strands"], rep["eligible"], rep["nonfinite"], rep["clusters_asked"]) == (N, int(ok.sum()), int((~ok).sum()), k)
    assert rep["clusters_made"] == res.guide.shape[0] and rep["clusters_made"] - rep["clusters_empty"] == G
    assert rep["iterations"] == res.iterations and rep["converged"] == res.converged and rep["total_last"] <= rep["total_first"]
    if G:
        assert rep["size_min"] == binding["cluster_size"].min() and rep["size_max"] == binding["cluster_size"].max()
        assert rep["distance_max"] == binding["strand_distance"][ok].max()


# ---- the library -------------------------------------------------------------------------------------------------------------------
FUNCTIONS = (("hgs_guides_assign", 13), ("hgs_guides_update", 12), ("hgs_guides_pick", 8))


def test_header_signatures_and_library_have_the_three_functions():
    import hgs_runtime as rt
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hgs.h")).read(), flags=re.S)
    L = rt.lib()
    for name, n_args in FUNCTIONS:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name
        assert decl.group(1).split(",")[0].strip() == "void* stream"
        assert name in rt.SIGNATURES and len(rt.SIGNATURES[name][1]) == n_args and hasattr(L, name), name
    assert L.hgs_abi_version() == 15


def test_entry_points_refuse_bad_arguments():
    """Nothing is launched: these run without a GPU (non-null arguments are the addresses of host buffers that are never read)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    bufs = [C.addressof(C.create_string_buffer(64)) for _ in range(8)]
    pts, st, cent, prev, lab, d2, chg, aux = bufs

    def assign(N=4, M=5, S=3, P=20, points=pts, status=st, K=2, c=cent, p=prev, l=lab, d=d2, ch=chg):
        return L.hgs_guides_assign(None, N, M, S, P, points, status, K, c, p, l, d, ch), L.hgs_last_error().decode()

    def update(N=4, M=5, S=3, P=20, points=pts, K=2, order=st, n=4, start=prev, c=cent, count=lab):
        return L.hgs_guides_update(None, N, M, S, P, points, K, order, n, start, c, count), L.hgs_last_error().decode()

    def pick(N=4, K=2, order=st, n=4, start=prev, d=d2, guide=aux):
        return L.hgs_guides_pick(None, N, K, order, n, start, d, guide), L.hgs_last_error().decode()

    shared = ((dict(N=-1), "bad sizes"), (dict(K=0), "K = 0"), (dict(K=65537), "K = 65537"))
    strands = ((dict(P=-1), "bad sizes"), (dict(M=1), "M = 1"), (dict(S=1), "S = 1"), (dict(S=65, M=100, P=400), "S = 65"), (dict(S=6), "S = 6"),
               (dict(P=19), "the point array holds 19"), (dict(N=2 ** 31 - 1, M=2 ** 31 - 1, P=2 ** 40), "the point array holds"),
               (dict(points=None), "null"))
    for call, name, more in ((assign, "hgs_guides_assign", strands + ((dict(status=None), "null"), (dict(c=None), "null"), (dict(l=None), "null"),
                                                                       (dict(d=None), "null"), (dict(ch=None), "null"), (dict(l=prev), "alias"),
                                                                       (dict(l=st), "alias"))),
                             (update, "hgs_guides_update", strands + ((dict(n=-1), "member list"), (dict(n=5), "member list"), (dict(order=None), "null"),
                                                                       (dict(start=None), "null"), (dict(c=None), "null"), (dict(count=None), "null"))),
                             (pick, "hgs_guides_pick", ((dict(n=-1), "member list"), (dict(n=5), "member list"), (dict(order=None), "null"),
                                                         (dict(start=None), "null"), (dict(d=None), "null"), (dict(guide=None), "null")))):
        for kw, words in shared + more:
            code, msg = call(**kw)
            assert code == 1 and name in msg and words in msg, (name, kw, msg)
    # no strand is not an error for the assignment, and no pointer is looked at; bad parameters are refused even then
    assert L.hgs_guides_assign(None, 0, 2, 2, 0, None, None, 1, None, None, None, None, None) == 0
    assert assign(N=0, S=1)[0] == 1 and assign(N=0, K=0)[0] == 1


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def test_driver_selects_guides(tmp_path, capsys):
    import export_strands
    from data import strand_files as F
    from scene.strand_guides import select_guides
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    common = ["-m", str(model), "--device", "cpu", "--points", "9", "--format", "hair", "--format", "usc", "--format", "npz", "--interpolate"]
    capsys.readouterr()
    plain, pp = export_strands.main(common + ["-o", str(tmp_path / "plain")])
    assert "Selected guides" not in capsys.readouterr().out and set(pp) == {"hair", "usc", "npz"}
    # without the flag its knobs change nothing
    _, kp = export_strands.main(common + ["-o", str(tmp_path / "knobs"), "--select_samples", "4", "--select_iters", "2"])
    capsys.readouterr()
    res, rp = export_strands.main(common + ["-o", str(tmp_path / "sel"), "--select_guides", "5", "--select_samples", "4", "--select_iters", "6"])
    text = capsys.readouterr().out
    line = [t for t in text.splitlines() if t.startswith("Selected guides")]
    assert len(line) == 1 and text.index("Interpolated:") < text.index("Selected guides") < text.index("Saved hair")
    for f in ("hair", "usc", "npz"):                                              # the main files: byte for byte
        assert open(pp[f], "rb").read() == open(kp[f], "rb").read() == open(rp[f], "rb").read(), f
    assert GR.same_bytes(res.points, plain.points) and res.n_strands == plain.n_strands == 29
    guides, binding, rep = select_guides(plain, 5, samples=4, iters=6)
    assert f"{guides.n_strands} guides from 29 of 29 strands" in line[0] and 1 <= guides.n_strands <= 5
    assert rp["hair_guides"] == str(tmp_path / "sel_guides.hair") and rp["usc_guides"] == str(tmp_path / "sel_guides.data")
    assert rp["npz_guides"] == str(tmp_path / "sel_guides.npz") and rp["guide_binding"] == str(tmp_path / "sel_guide_binding.npz")
    F.write_strands_cy(str(tmp_path / "want.hair"), guides)
    F.write_strands_usc(str(tmp_path / "want.data"), guides)
    assert open(rp["hair_guides"], "rb").read() == open(tmp_path / "want.hair", "rb").read()
    assert open(rp["usc_guides"], "rb").read() == open(tmp_path / "want.data", "rb").read()
    with np.load(rp["guide_binding"]) as z:
        assert set(z.files) == {"guide_strand", "strand_guide", "strand_distance", "cluster_size", "k", "samples", "iterations", "converged"}
        for key, want in binding.items():
            assert GR.same_bytes(z[key], want), key
        assert int(z["k"]) == 5 and int(z["samples"]) == 4 and int(z["iterations"]) == rep["iterations"] and bool(z["converged"]) == rep["converged"]
        assert np.array_equal(z["strand_guide"][z["guide_strand"]], np.arange(guides.n_strands))


def test_driver_refuses_bad_values(tmp_path, capsys):
    import export_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    for bad, words in ((["--select_guides", "0"], "k = 0"), (["--select_guides", "65537"], "k = 65537"),
                       (["--select_guides", "3", "--select_samples", "1"], "samples"), (["--select_guides", "3", "--select_samples", "65"], "samples"),
                       (["--select_guides", "3", "--select_iters", "0"], "iters"), (["--select_guides", "3", "--points", "0"], "--points M > 0 is needed")):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x")] + bad)
        err = capsys.readouterr().err
        assert stop.value.code == 2 and "export_strands.py: --select_guides" in err and words in err, bad
    assert not (tmp_path / "x.hair").exists()
