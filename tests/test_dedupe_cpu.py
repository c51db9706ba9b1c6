"""The strand deduplication on the CPU (scene/strand_dedupe.py numpy path, export_strands.py --dedupe): the vectorised path against the
loop restatement of the contract (tests/dedupe_reference.py) bit for bit on the cases of tests/dedupe_cases.py, the contract's
consequences (an independent kept set, every dropped strand beside its kept_by, idempotence, tol = 0, the chain), the report, the
refusals, the C entry points' refusals (which launch nothing) and the driver.  Every comparison is of bytes or of integers: no numeric
tolerance is involved."""
import functools

import numpy as np
import pytest

from tests import dedupe_cases as DC
from tests import dedupe_reference as DR

FIELDS = ("keep", "kept_by", "rounds", "lower_offsets", "lower")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of one case: (keep, kept_by, rounds, lower_offsets, lower); computed once, shared with the GPU tests."""
    return DR.dedupe(*DC.cases()[name])


def assert_same(got, ref, what):
    for name, a, b in zip(FIELDS, got, ref):
        assert DR.same_bytes(np.asarray(a), b), (what, name)


def export_of(pts, off, attrs=None):
    from scene.strand_export import StrandExport
    N = off.shape[0] - 1
    attrs = np.arange(pts.shape[0] * 2, dtype=np.float32).reshape(-1, 2) if attrs is None else attrs
    return StrandExport(pts, attrs, off, np.arange(N, dtype=np.int64) + 5, np.arange(N, dtype=np.float64) * 0.5)


@pytest.mark.parametrize("name", DC.NAMES)
def test_numpy_path_matches_the_loop_restatement(name):
    from scene.strand_dedupe import dedupe_numpy
    got = dedupe_numpy(*DC.cases()[name])
    assert_same(got, reference(name), name)
    # a budget that cuts the root test into blocks of a few strands, and the joint test into a few pairs, changes nothing
    assert_same(dedupe_numpy(*DC.cases()[name], budget=1500), reference(name), name + " (small blocks)")


@pytest.mark.parametrize("M", DC.MS)
@pytest.mark.parametrize("N", DC.NS)
def test_numpy_path_at_every_strand_count(N, M):
    from scene.strand_dedupe import dedupe_numpy
    pts, off, tol = DC.cases()[f"blob_m{M}"]
    assert_same(dedupe_numpy(*DC.first_strands(pts, off, N), tol), DR.cut(reference(f"blob_m{M}"), N), f"N={N} M={M}")


def test_the_cases_exercise_what_they_are_meant_to():
    """The restatement's own results say that every branch of the contract is taken."""
    for M in DC.MS:
        keep, kept_by, rounds, starts, lower = reference(f"blob_m{M}")
        pts, off, tol = DC.cases()[f"blob_m{M}"]
        assert 60 < len(lower) < 400 and rounds.max() >= 3 and 0 < (keep == 0).sum() < 200
        roots = pts[off[:-1]].astype(np.float64)
        close = sum(1 for i in range(1, 513) for j in np.nonzero(((roots[:i] - roots[i]) ** 2).sum(1) <= tol * tol)[0])
        assert close > len(lower) + (10 if M > 2 else 0)                            # roots that pass, strands that do not: the planted moved joints
    for name in ("tip", "root"):
        keep, kept_by, rounds, starts, lower = reference(name)
        assert keep.tolist() == [1, 0, 1, 0, 0] * 6 and kept_by[:5].tolist() == [0, 0, 2, 0, 2]
    keep, kept_by, _, starts, lower = reference("boundary")
    assert [int(starts[2 * k + 3] - starts[2 * k + 2]) == 1 for k in range(6)] == DC.BOUNDARY_PAIRS and starts[-1] == 3
    keep, kept_by, rounds, _, _ = reference("exact")
    assert keep.tolist() == [1, 0, 1, 0, 1, 0, 0] and kept_by.tolist() == [0, 0, 2, 0, 4, 2, 4]     # one bit apart is no copy; -0.0 is 0.0
    for name, n in (("identical", 130), ("identical_tol0", 70)):
        keep, kept_by, rounds, starts, lower = reference(name)
        assert len(lower) == n * (n - 1) // 2 and keep.sum() == 1 and not kept_by.any() and rounds.tolist() == list(range(n))
    keep, kept_by, rounds, starts, lower = reference("chain")
    assert keep.tolist() == [1, 0] * 20 and rounds.tolist() == list(range(40)) and lower.tolist() == list(range(39))
    assert kept_by.tolist() == [c - (c % 2) for c in range(40)]
    keep, kept_by, rounds, starts, lower = reference("nonfinite")
    pts, off, tol = DC.cases()["nonfinite"]
    bad = ~np.isfinite(pts.reshape(30, -1)).all(axis=1)
    assert bad.sum() == 20 and keep[bad].all() and not rounds[bad].any() and not np.isin(lower, np.nonzero(bad)[0]).any()
    assert keep[~bad].sum() == 1 and (starts[1:] - starts[:-1])[bad].sum() == 0


@pytest.mark.parametrize("name", DC.NAMES)
def test_consequences_of_the_contract(name):
    """No two kept strands pair, every dropped strand pairs with its kept_by, which is kept and earlier, the kept strands keep every bit,
    and the step on its own output drops nothing."""
    from scene.strand_dedupe import dedupe_numpy, dedupe_strands
    pts, off, tol = DC.cases()[name]
    res = dedupe_numpy(pts, off, tol)
    kept = np.nonzero(res.keep)[0]
    N = off.shape[0] - 1
    if N <= 130:                                                                    # (the blobs: by the lists, which the restatement vouches for)
        assert not any(DR.pair(pts, off, tol, int(i), int(j)) for a, i in enumerate(kept) for j in kept[:a])
    for i in range(N):
        mine = res.lower[res.lower_offsets[i]:res.lower_offsets[i + 1]]
        assert np.all(mine[1:] > mine[:-1]) and np.all(mine < i)
        if res.keep[i]:
            assert res.kept_by[i] == i and not res.keep[mine].any()
        else:
            j = int(res.kept_by[i])
            assert j < i and res.keep[j] and j == mine[res.keep[mine] != 0][0] and DR.pair(pts, off, tol, i, j)
    strands = export_of(pts, off)
    out, rep = dedupe_strands(strands, tol)
    M = int(off[1] - off[0])
    rows = (off[kept][:, None] + np.arange(M)[None, :]).reshape(-1)
    assert DR.same_bytes(out.points, pts[rows]) and DR.same_bytes(out.attrs, strands.attrs[rows])
    assert DR.same_bytes(out.offsets, np.arange(len(kept) + 1, dtype=np.int64) * M)
    assert DR.same_bytes(out.strand_ids, strands.strand_ids[kept]) and DR.same_bytes(out.length, strands.length[kept])
    again, rep2 = dedupe_strands(out, tol)
    assert rep2["dropped"] == 0 and rep2["pairs"] == 0 and rep2["rounds"] == 0 and all(DR.same_bytes(a, b) for a, b in zip(again, out))
    assert rep["kept"] == len(kept) == rep2["strands"] and rep["joints_after"] == len(kept) * M


def test_report_on_the_known_cases():
    from scene.strand_dedupe import dedupe_strands
    _, rep = dedupe_strands(export_of(*DC.cases()["identical"][:2]), DC.TOL)
    assert rep == dict(strands=130, kept=1, dropped=129, nonfinite=0, pairs=8385, rounds=129, groups=1, largest_group=129, joints_before=390,
                       joints_after=3)
    _, rep = dedupe_strands(export_of(*DC.cases()["chain"][:2]), 1.0)
    assert rep == dict(strands=40, kept=20, dropped=20, nonfinite=0, pairs=39, rounds=39, groups=20, largest_group=1, joints_before=120,
                       joints_after=60)
    _, rep = dedupe_strands(export_of(*DC.cases()["nonfinite"][:2]), DC.TOL)
    assert (rep["strands"], rep["kept"], rep["nonfinite"], rep["groups"], rep["largest_group"]) == (30, 21, 20, 1, 9)
    _, rep = dedupe_strands(export_of(*DC.cases()["tip"][:2]), DC.TOL)
    assert (rep["kept"], rep["dropped"], rep["groups"], rep["largest_group"], rep["rounds"]) == (12, 18, 12, 2, 2)
    from scene.strand_export import StrandExport
    none = StrandExport(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    out, rep = dedupe_strands(none, 0.5)
    assert out.n_strands == 0 and rep == dict(strands=0, kept=0, dropped=0, nonfinite=0, pairs=0, rounds=0, groups=0, largest_group=0,
                                              joints_before=0, joints_after=0)


def test_one_round_is_what_the_loop_is_made_of():
    """resolve_round_numpy from a handed-in state that mixes decided and undecided strands: only the undecided strands whose lower
    neighbours are all decided change, and kept_by and rounds are written for them alone."""
    from scene.strand_dedupe import DROPPED, KEPT, UNDECIDED, resolve_round_numpy
    _, _, _, starts, lower = reference("chain")
    state = np.array([KEPT, UNDECIDED, KEPT, UNDECIDED, UNDECIDED, DROPPED, UNDECIDED] + [UNDECIDED] * 33, np.uint8)
    kept_by, rounds = np.full(40, -7, np.int64), np.full(40, -7, np.int32)
    out, left = resolve_round_numpy(starts, lower, state, kept_by, rounds, 5)
    assert out[:8].tolist() == [KEPT, DROPPED, KEPT, DROPPED, UNDECIDED, DROPPED, KEPT, UNDECIDED] and left == 34
    assert kept_by[:8].tolist() == [-7, 0, -7, 2, -7, -7, 6, -7] and rounds[:8].tolist() == [-7, 5, -7, 5, -7, -7, 5, -7]


def test_refusals(monkeypatch):
    from scene import strand_dedupe as SD
    for bad in DC.REFUSED:
        with pytest.raises(ValueError, match="tol"):
            SD.check_parameters(bad)
    assert SD.check_parameters(0) == 0.0 and SD.check_parameters(np.float32(0.5)) == 0.5 and isinstance(SD.check_parameters(1), float)
    pts, off, tol = DC.cases()["tip"]
    with pytest.raises(ValueError, match="tol"):
        SD.dedupe_numpy(pts, off, -1.0)
    with pytest.raises(ValueError, match="same number"):                              # ragged
        SD.dedupe_numpy(pts[:-1], np.append(off[:-1], off[-1] - 1), tol)
    with pytest.raises(ValueError, match="same number"):                              # M = 1
        SD.dedupe_numpy(pts[:7], np.arange(8, dtype=np.int64), tol)
    with pytest.raises(ValueError, match="same number"):
        SD.dedupe_strands(export_of(pts[:7], np.arange(8, dtype=np.int64)), tol)
    for bad in (off[1:], off[:-1], off.astype(np.float64)):
        with pytest.raises(ValueError, match="offsets"):
            SD.dedupe_numpy(pts, bad, tol)
    with pytest.raises(ValueError, match="points"):
        SD.dedupe_numpy(pts.reshape(-1), off, tol)
    with pytest.raises(ValueError, match="device"):
        SD.dedupe_strands(export_of(pts, off), tol, device="cpu")
    pts, off, tol = DC.cases()["identical"]
    monkeypatch.setattr(SD, "MAX_PAIRS", 8385)                                      # exactly the case's list: allowed
    assert SD.dedupe_numpy(pts, off, tol).lower.shape[0] == 8385
    monkeypatch.setattr(SD, "MAX_PAIRS", 8384)
    with pytest.raises(ValueError, match="^8385 pairs.*above the 8384.*smaller"):       # the refusal names the pairs there are, as the device path's does
        SD.dedupe_numpy(pts, off, tol)
    with pytest.raises(ValueError, match="^8385 pairs"):
        SD.dedupe_numpy(pts, off, tol, budget=1500)                                 # (refused in an early block, counted to the end)
    with pytest.raises(ValueError, match="smaller"):
        SD.dedupe_strands(export_of(pts, off), tol)


# ---- the entry points' refusals ------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    """Nothing is launched: these run without a GPU (non-null arguments are the addresses of host buffers that are never read)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    bufs = [C.create_string_buffer(64) for _ in range(8)]
    pts, cnt, st, low, off, s_in, s_out, kb = (C.addressof(b) for b in bufs)
    rd, word = C.addressof(bufs[1]) + 32, C.addressof(bufs[2]) + 32
    nan, inf = float("nan"), float("inf")

    def count(N=2, M=3, P=6, points=pts, tol=0.5, counts=cnt):
        return L.hgs_dedupe_count(None, N, M, P, points, tol, counts), L.hgs_last_error().decode()

    def fill(N=2, M=3, P=6, points=pts, tol=0.5, starts=st, n_pairs=1, lower=low):
        return L.hgs_dedupe_fill(None, N, M, P, points, tol, starts, n_pairs, lower), L.hgs_last_error().decode()

    def resolve(N=2, offsets=off, n_pairs=1, lower=low, state=s_in, state_out=s_out, r=1, kept_by=kb, rounds=rd, undecided=word):
        return L.hgs_dedupe_resolve(None, N, offsets, n_pairs, lower, state, state_out, r, kept_by, rounds, undecided), L.hgs_last_error().decode()

    search = ((dict(N=-1), "bad sizes"), (dict(P=-1), "bad sizes"), (dict(M=1), "M = 1"), (dict(M=0), "M = 0"), (dict(P=5), "point array"),
              (dict(tol=-1.0), "tol"), (dict(tol=nan), "tol"), (dict(tol=inf), "tol"), (dict(tol=-inf), "tol"), (dict(points=None), "null"))
    for fn, name, more in ((count, "hgs_dedupe_count", ((dict(counts=None), "null"), (dict(counts=pts), "alias"))),
                           (fill, "hgs_dedupe_fill", ((dict(starts=None), "null"), (dict(lower=None), "null"), (dict(n_pairs=-1), "bad sizes"),
                                                      (dict(lower=pts), "alias"), (dict(lower=st), "alias"), (dict(starts=pts), "alias")))):
        for kw, words in search + more:
            code, msg = fn(**kw)
            assert code == 1 and name in msg and words in msg, (name, kw, msg)
    for kw, words in ((dict(N=-1), "bad sizes"), (dict(n_pairs=-1), "bad sizes"), (dict(r=0), "round"), (dict(r=-3), "round"), (dict(offsets=None), "null"),
                      (dict(lower=None), "null"), (dict(state=None), "null"), (dict(state_out=None), "null"), (dict(kept_by=None), "null"),
                      (dict(rounds=None), "null"), (dict(undecided=None), "null"), (dict(state_out=s_in), "alias"), (dict(kept_by=off), "alias"),
                      (dict(rounds=low), "alias"), (dict(undecided=rd), "alias"), (dict(rounds=kb), "alias")):
        code, msg = resolve(**kw)
        assert code == 1 and "hgs_dedupe_resolve" in msg and words in msg, (kw, msg)
    # nothing to do is not an error, and no pointer is looked at; a bad tolerance is refused even then
    assert L.hgs_dedupe_count(None, 0, 2, 0, None, 0.0, None) == 0
    assert L.hgs_dedupe_fill(None, 0, 2, 0, None, 0.0, None, 0, None) == 0
    assert L.hgs_dedupe_fill(None, 2, 3, 6, None, 0.0, None, 0, None) == 0        # no pairs: nothing to fill
    assert L.hgs_dedupe_resolve(None, 0, None, 0, None, None, None, 1, None, None, None) == 0
    assert count(N=0, tol=nan)[0] == 1 and fill(N=0, tol=-1.0)[0] == 1 and count(N=0, M=1)[0] == 1


# ---- the driver --------------------------------------------------------------------------------------------------------------------
DRIVER_DIST = "1e-4"


def driver_args(model):
    return ["-m", str(model), "--device", "cpu", "--points", "9", "--format", "hair", "--format", "usc"]


def written_hashes(paths):
    """sha256 of every written file; of an .npz (whose container carries the time of writing) the arrays' names, types, shapes and bytes."""
    import hashlib
    out = {}
    for key, p in paths.items():
        if p.endswith(".npz"):
            h = hashlib.sha256()
            with np.load(p) as f:
                for name in sorted(f.files):
                    h.update(name.encode() + str(f[name].dtype).encode() + str(f[name].shape).encode() + f[name].tobytes())
            out[key] = h.hexdigest()
        else:
            out[key] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def test_driver_without_the_flag_writes_the_bytes_it_wrote_before(tmp_path, capsys):
    """tests/golden/dedupe_driver_before.json holds the hashes of what this command wrote at the commit before --dedupe existed."""
    import json
    import os
    import export_strands
    from data import strand_files as F
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    common = driver_args(model) + ["--interpolate", "--select_guides", "5", "--select_samples", "4", "--simplify", "2e-4"]
    a, pa = export_strands.main(common + ["-o", str(tmp_path / "a")])
    text = capsys.readouterr().out
    assert "Deduplicated" not in text
    with open(os.path.join(os.path.dirname(__file__), "golden", "dedupe_driver_before.json")) as f:
        before = json.load(f)["sha256"]
    assert written_hashes(pa) == before
    F.write_strands_cy(str(tmp_path / "was.hair"), a)                               # the writers on the chain's strands: nothing was taken out
    assert open(pa["hair"], "rb").read() == open(tmp_path / "was.hair", "rb").read() and a.n_strands == 29


def test_driver_drops_the_copies_the_interpolation_makes(tmp_path, capsys):
    import export_strands
    from data import strand_files as F
    from scene.strand_dedupe import dedupe_numpy, dedupe_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    common = driver_args(model) + ["--interpolate"]
    plain, _ = export_strands.main(common + ["-o", str(tmp_path / "plain")])
    capsys.readouterr()
    res, paths = export_strands.main(common + ["-o", str(tmp_path / "dd"), "--dedupe", DRIVER_DIST])
    text = capsys.readouterr().out
    want, rep = dedupe_strands(plain, float(DRIVER_DIST))
    line = [t for t in text.splitlines() if t.startswith("Deduplicated strands (dist 0.0001): ")]
    assert len(line) == 1 and f"{rep['kept']} of {rep['strands']} strands kept" in line[0] and f"{rep['pairs']} pairs" in line[0]
    assert text.index("Interpolated:") < text.index("Deduplicated strands") < text.index("Saved hair")
    assert res.n_strands == rep["kept"] and 7 <= rep["kept"] <= 22 and rep["strands"] == 29    # every guide's root is a root: 7 copies at the least
    for a, b in zip(res, want):
        assert DR.same_bytes(a, b)
    assert DR.same_bytes(res.points[:63], plain.points[:63]) and res.strand_ids[:7].tolist() == list(range(7))      # the trained strands all survive
    pts, off = F.read_usc_hair(paths["usc"])
    assert DR.same_bytes(pts, want.points) and off.shape[0] - 1 == rep["kept"]
    again = dedupe_numpy(pts, off, float(DRIVER_DIST))
    assert again.keep.all() and again.lower.shape[0] == 0                           # no two written strands pair


def test_driver_selects_guides_among_the_deduplicated_strands(tmp_path, capsys):
    import export_strands
    from scene.strand_guides import select_guides
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    common = driver_args(model) + ["--interpolate", "--dedupe", DRIVER_DIST]
    plain, _ = export_strands.main(common + ["-o", str(tmp_path / "plain")])
    capsys.readouterr()
    res, paths = export_strands.main(common + ["-o", str(tmp_path / "g"), "--select_guides", "5", "--select_samples", "4", "--simplify", "2e-4"])
    text = capsys.readouterr().out
    assert text.index("Deduplicated strands") < text.index("Selected guides") < text.index("Simplified strands")
    _, binding, _ = select_guides(plain, 5, samples=4)
    with np.load(paths["guide_binding"]) as f:
        assert f["strand_guide"].shape[0] == plain.n_strands == res.n_strands < 29
        assert DR.same_bytes(f["guide_strand"], binding["guide_strand"]) and DR.same_bytes(f["strand_guide"], binding["strand_guide"])
        assert int(f["guide_strand"].max()) < res.n_strands


def test_driver_refuses_bad_values(tmp_path, capsys, monkeypatch):
    import export_strands
    from scene import strand_dedupe as SD
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    for bad in ("-1", "nan", "inf", "-inf"):
        with pytest.raises(SystemExit) as stop:
            export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), f"--dedupe={bad}"])
        assert stop.value.code == 2 and "export_strands.py: --dedupe" in capsys.readouterr().err, bad
    with pytest.raises(SystemExit) as stop:
        export_strands.main(["-m", str(model), "--device", "cpu", "-o", str(tmp_path / "x"), "--points", "0", "--dedupe", DRIVER_DIST])
    err = capsys.readouterr().err
    assert stop.value.code == 2 and "export_strands.py: --dedupe" in err and "--points M > 0 is needed" in err
    plain, _ = export_strands.main(driver_args(model) + ["--interpolate", "-o", str(tmp_path / "plain")])
    pairs = SD.dedupe_strands(plain, float(DRIVER_DIST))[1]["pairs"]
    capsys.readouterr()
    monkeypatch.setattr(SD, "MAX_PAIRS", 3)
    with pytest.raises(SystemExit) as stop:
        export_strands.main(driver_args(model) + ["--interpolate", "-o", str(tmp_path / "x"), "--dedupe", DRIVER_DIST])
    err = capsys.readouterr().err
    assert pairs > 3 and stop.value.code == 2 and f"export_strands.py: --dedupe: {pairs} pairs" in err and "smaller" in err
    assert not (tmp_path / "x.hair").exists()
