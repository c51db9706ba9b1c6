"""The strand deduplication on the GPU (csrc/hgs_dedupe.hip through scene/strand_dedupe.py): the kernels against the numpy path and the
loop restatement of the contract (tests/dedupe_reference.py) bit for bit on the cases and strand counts of tests/dedupe_cases.py, each
kernel alone (count and fill, one resolve round from a handed-in state), a second run, the wrapper's checks, the C entry
points' refusals on device buffers, and the driver on both devices."""
import numpy as np
import pytest
import torch

from tests import dedupe_cases as DC
from tests import dedupe_reference as DR
from tests.test_dedupe_cpu import DRIVER_DIST, assert_same, driver_args, export_of, reference, written_hashes

pytestmark = pytest.mark.gpu


def _up(pts, off):
    return torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")


def _device(pts, off, tol, **kw):
    from scene.strand_dedupe import dedupe_device
    return tuple(t.cpu().numpy() for t in dedupe_device(*_up(pts, off), tol, **kw))


@pytest.mark.parametrize("name", DC.NAMES)
def test_kernels_match_the_numpy_path_and_the_restatement(name):
    from scene.strand_dedupe import dedupe_numpy, dedupe_strands
    pts, off, tol = DC.cases()[name]
    got = _device(pts, off, tol)
    assert_same(got, dedupe_numpy(pts, off, tol), name + " (numpy)")
    assert_same(got, reference(name), name + " (loops)")
    assert_same(_device(pts, off, tol), got, name + " (a second run)")
    strands = export_of(pts, off)
    host, hr = dedupe_strands(strands, tol)
    dev, dr = dedupe_strands(strands, tol, device="cuda")
    assert dr == hr and all(DR.same_bytes(a, b) for a, b in zip(dev, host)), (name, dr, hr)


@pytest.mark.parametrize("M", DC.MS)
def test_kernels_at_every_strand_count(M):
    pts, off, tol = DC.cases()[f"blob_m{M}"]
    for N in DC.NS:
        assert_same(_device(*DC.first_strands(pts, off, N), tol), DR.cut(reference(f"blob_m{M}"), N), f"N={N} M={M}")


@pytest.mark.parametrize("name", ("blob_m3", "blob_m100", "identical", "chain", "nonfinite"))
def test_count_and_fill_alone(name):
    """counts [N, DEDUPE_PARTS]: every row sums to the strand's lower neighbours, and the flattened prefix sums place the parts so that
    the fill pass writes the lists whole and ascending, and nothing behind them."""
    import hgs_runtime as rt
    from scene.strand_dedupe import count_device, fill_device, pairs_device
    pts, off, tol = DC.cases()[name]
    _, _, _, starts, lower = reference(name)
    N, M = off.shape[0] - 1, int(off[1] - off[0])
    p = torch.as_tensor(pts, device="cuda")
    counts = count_device(p, N, M, tol)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (N, rt.DEDUPE_PARTS)
    assert np.array_equal(counts.sum(dim=1).cpu().numpy(), starts[1:] - starts[:-1])
    st = torch.cumsum(counts.view(-1), 0, dtype=torch.int64) - counts.view(-1)
    assert DR.same_bytes(st[::rt.DEDUPE_PARTS].cpu().numpy(), starts[:-1])
    filled = torch.full((len(lower) + 8,), -7, dtype=torch.int32, device="cuda")           # (the entries behind the list stay as they are)
    rt.check(rt.lib().hgs_dedupe_fill(rt.current_stream(), N, M, pts.shape[0], p.data_ptr(), tol, st.data_ptr(), len(lower), filled.data_ptr()))
    got = filled.cpu().numpy()
    assert DR.same_bytes(got[:len(lower)], lower) and (got[len(lower):] == -7).all()
    assert DR.same_bytes(fill_device(p, N, M, tol, st, len(lower)).cpu().numpy(), lower)
    o, l = pairs_device(p, N, M, tol)
    assert DR.same_bytes(o.cpu().numpy(), starts) and DR.same_bytes(l.cpu().numpy(), lower)


def test_fill_never_writes_past_a_slot_that_is_too_small():
    """A fill whose tol finds more pairs than its starts leave room for (another tol than the count's) stops at every slot's end."""
    import hgs_runtime as rt
    pts, off, tol = DC.cases()["identical"]
    N, M = 130, 3
    p = torch.as_tensor(pts, device="cuda")
    starts = torch.arange(N, dtype=torch.int64, device="cuda").repeat_interleave(rt.DEDUPE_PARTS)      # one entry a strand, in its last part
    filled = torch.full((2 * N + 8,), -7, dtype=torch.int32, device="cuda")
    rt.check(rt.lib().hgs_dedupe_fill(rt.current_stream(), N, M, pts.shape[0], p.data_ptr(), tol, starts.data_ptr(), N - 1, filled.data_ptr()))
    got = filled.cpu().numpy()
    assert got[0] == -7 and not got[1:N - 1].any() and (got[N - 1:] == -7).all()        # strand 0 has none; the others wrote their first, 0 (one tile: the last part walks it); the last had no room


@pytest.mark.parametrize("name", ("chain", "blob_m3", "identical"))
def test_one_resolve_round_alone(name):
    """From a handed-in state that mixes decided and undecided strands, against the numpy statement of one round; the undecided word is
    added to what was there; kept_by and rounds are written for the strands the round decides and for no other."""
    from scene.strand_dedupe import KEPT, UNDECIDED, resolve_round_device, resolve_round_numpy
    _, _, _, starts, lower = reference(name)
    N = starts.shape[0] - 1
    rng = np.random.default_rng(5)
    state = rng.integers(0, 3, N).astype(np.uint8)
    state[0] = KEPT
    state[1::7] = UNDECIDED
    kept_by, rounds = np.full(N, -7, np.int64), np.full(N, -7, np.int32)
    want, left = resolve_round_numpy(starts, lower, state, kept_by, rounds, 9)
    assert 0 < left < N and (want != state).any()
    d = lambda a: torch.as_tensor(a, device="cuda")
    s_in, s_out = d(state), torch.full((N,), 77, dtype=torch.uint8, device="cuda")
    kb, rd = torch.full((N,), -7, dtype=torch.int64, device="cuda"), torch.full((N,), -7, dtype=torch.int32, device="cuda")
    word = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    resolve_round_device(d(starts), d(lower), s_in, s_out, 9, kb, rd, word)
    assert DR.same_bytes(s_out.cpu().numpy(), want) and DR.same_bytes(s_in.cpu().numpy(), state)
    assert DR.same_bytes(kb.cpu().numpy(), kept_by) and DR.same_bytes(rd.cpu().numpy(), rounds) and int(word) == 1000 + left


def test_resolve_from_the_lists_alone():
    from scene.strand_dedupe import resolve_device
    for name in ("identical", "chain", "nonfinite", "blob_m2"):
        keep, kept_by, rounds, starts, lower = reference(name)
        got = resolve_device(torch.as_tensor(starts, device="cuda"), torch.as_tensor(lower, device="cuda"))
        assert_same(tuple(t.cpu().numpy() for t in got), (keep, kept_by, rounds), name)


def test_more_pairs_than_the_lists_may_hold_are_refused(monkeypatch):
    import hgs_runtime as rt
    from scene import strand_dedupe as SD
    pts, off, tol = DC.cases()["identical"]
    monkeypatch.setattr(SD, "MAX_PAIRS", 8384)
    with pytest.raises(rt.HgsError, match="8385 pairs.*smaller"):
        SD.dedupe_device(*_up(pts, off), tol)
    with pytest.raises(rt.HgsError, match="smaller"):
        SD.dedupe_strands(export_of(pts, off), tol, device="cuda")


def test_device_wrapper_checks_its_tensors():
    import hgs_runtime as rt
    from scene.strand_dedupe import dedupe_device
    pts, off, tol = DC.cases()["tip"]
    pts_d, off_d = _up(pts, off)
    with pytest.raises(rt.HgsError):
        dedupe_device(torch.as_tensor(pts), off_d, tol)                             # a host tensor is not moved to the GPU behind the caller's back
    with pytest.raises(rt.HgsError):
        dedupe_device(pts_d, torch.as_tensor(off), tol)
    with pytest.raises(rt.HgsError):
        dedupe_device(pts_d, off_d.to(torch.int32), tol)
    with pytest.raises(rt.HgsError):
        dedupe_device(pts_d.to(torch.float64), off_d, tol)
    with pytest.raises(rt.HgsError, match="expected"):
        dedupe_device(pts_d.reshape(-1), off_d, tol)
    with pytest.raises(rt.HgsError, match="same number"):                           # ragged
        dedupe_device(pts_d[:-1], torch.cat([off_d[:-1], off_d[-1:] - 1]), tol)
    with pytest.raises(rt.HgsError, match="same number"):                           # M = 1
        dedupe_device(pts_d[:7], torch.arange(8, device="cuda"), tol)
    with pytest.raises(rt.HgsError, match="tile"):
        dedupe_device(pts_d, off_d[:-1], tol)
    for bad in DC.REFUSED:
        with pytest.raises(rt.HgsError, match="tol"):
            dedupe_device(pts_d, off_d, bad)
    empty = dedupe_device(pts_d[:0], off_d[:1], tol)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0,), (1,), (0,)] and empty.lower.dtype == torch.int32


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    """On device buffers: every refusal returns 1 and leaves the output buffers as they were."""
    import hgs_runtime as rt
    L = rt.lib()
    pts, off, tol = DC.cases()["tip"]
    _, _, _, starts, lower = reference("tip")
    N, M, P, n = 30, 5, pts.shape[0], len(lower)
    d = lambda a: torch.as_tensor(a, device="cuda")
    # (30 strands are one tile, which the last part walks: every strand's list begins and ends in its last slot)
    p, st, lo_off, lo = d(pts), d(np.repeat(starts[:-1], rt.DEDUPE_PARTS)), d(starts), d(lower)
    counts = torch.full((N, rt.DEDUPE_PARTS), -7, dtype=torch.int32, device="cuda")
    filled = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s_in = torch.zeros(N, dtype=torch.uint8, device="cuda")
    s_out = torch.full((N,), 77, dtype=torch.uint8, device="cuda")
    kb, rd = torch.full((N,), -7, dtype=torch.int64, device="cuda"), torch.full((N,), -7, dtype=torch.int32, device="cuda")
    word = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    nan, inf = float("nan"), float("inf")

    def count(N_=N, M_=M, P_=P, points=p.data_ptr(), tol_=tol, c=counts.data_ptr()):
        return L.hgs_dedupe_count(rt.current_stream(), N_, M_, P_, points, tol_, c)

    def fill(N_=N, M_=M, P_=P, points=p.data_ptr(), tol_=tol, starts_=st.data_ptr(), n_=n, low=filled.data_ptr()):
        return L.hgs_dedupe_fill(rt.current_stream(), N_, M_, P_, points, tol_, starts_, n_, low)

    def resolve(N_=N, offsets=lo_off.data_ptr(), n_=n, low=lo.data_ptr(), a=s_in.data_ptr(), b=s_out.data_ptr(), r=1, k=kb.data_ptr(), rr=rd.data_ptr(),
                w=word.data_ptr()):
        return L.hgs_dedupe_resolve(rt.current_stream(), N_, offsets, n_, low, a, b, r, k, rr, w)

    search = (dict(N_=-1), dict(P_=-1), dict(M_=1), dict(P_=P - 1), dict(tol_=-1.0), dict(tol_=nan), dict(tol_=inf), dict(points=None))
    for kw in search + (dict(c=None), dict(c=p.data_ptr())):
        assert count(**kw) == 1 and b"hgs_dedupe_count" in L.hgs_last_error(), kw
    for kw in search + (dict(starts_=None), dict(low=None), dict(n_=-1), dict(low=p.data_ptr()), dict(low=st.data_ptr())):
        assert fill(**kw) == 1 and b"hgs_dedupe_fill" in L.hgs_last_error(), kw
    for kw in (dict(N_=-1), dict(n_=-1), dict(r=0), dict(offsets=None), dict(low=None), dict(a=None), dict(b=None), dict(k=None), dict(rr=None),
               dict(w=None), dict(b=s_in.data_ptr()), dict(k=lo_off.data_ptr()), dict(rr=lo.data_ptr())):
        assert resolve(**kw) == 1 and b"hgs_dedupe_resolve" in L.hgs_last_error(), kw
    assert count(N_=0, P_=0) == 0 and fill(N_=0, P_=0) == 0 and fill(n_=0) == 0 and resolve(N_=0) == 0
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((filled == -7).all()) and bool((s_out == 77).all()) and bool((kb == -7).all())
    assert bool((rd == -7).all()) and int(word) == 5
    assert count() == 0 and fill() == 0
    torch.cuda.synchronize()
    assert DR.same_bytes(counts.sum(dim=1).cpu().numpy(), starts[1:] - starts[:-1]) and DR.same_bytes(filled.cpu().numpy(), lower)


def test_driver_on_both_devices_writes_identical_files(tmp_path, capsys):
    import export_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    extra = ["--interpolate", "--dedupe", DRIVER_DIST, "--select_guides", "5", "--select_samples", "4", "--simplify", "2e-4"]
    host, hp = export_strands.main(driver_args(model) + extra + ["-o", str(tmp_path / "host")])
    capsys.readouterr()
    dev, dp = export_strands.main([a if a != "cpu" else "cuda" for a in driver_args(model)] + extra + ["-o", str(tmp_path / "dev")])
    line = [t for t in capsys.readouterr().out.splitlines() if t.startswith("Deduplicated strands")]
    assert len(line) == 1 and dev.n_strands == host.n_strands < 29
    assert set(hp) == set(dp) and len(hp) == 5
    assert written_hashes(hp) == written_hashes(dp)
