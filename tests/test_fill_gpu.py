"""hgs_field_fill (csrc/hgs_fill.hip) against the numpy path of utils/field_fill.py and the loop restatement of tests/fill_reference.py:
every tensor entry of both returned iterates bit for bit, at free-node counts around the wavefront and the workgroup, repeated and on
a side stream; nothing written outside the FREE nodes; the analytic line; quantise, the device solve and merge against the numpy path
under trace_reference.compare_solves; the wrapper's refusals; and the trace_strands.py --fill driver on both devices."""
import numpy as np
import pytest
import torch

from tests import fill_cases as FC
from tests import trace_reference as TR
from tests.test_fill_cpu import BOX, check_against_loop, kind_counts, same_bits
from tests.test_trace_cpu import DRIVER
from utils import field_fill as FF
from utils import trace as T

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fill_dev(T0, kind, sweeps):
    res, prev = FF.fill_device(_dev(T0), _dev(kind), sweeps)
    return res.cpu().numpy(), prev.cpu().numpy()


@pytest.mark.parametrize("grid", list(FC.GRIDS))
@pytest.mark.parametrize("name", FC.PATTERNS)
def test_fill_equals_the_restatement_and_the_numpy_path(name, grid):
    shape = FC.GRIDS[grid]
    _, kind, T0 = FC.pattern(name, shape)
    its = check_against_loop(fill_dev, (name, grid), T0, kind, FC.SWEEPS_GPU)
    for n in FC.SWEEPS_GPU:
        host = FF.fill_numpy(T0, kind, n)
        assert same_bits(host[0], its[n]) and same_bits(host[1], its[max(n - 1, 0)])
    res, prev = FF.fill(T0, kind, 7, device="cuda")              # the host-array entry point
    assert same_bits(res, its[7]) and same_bits(prev, its[6])


@pytest.mark.parametrize("F", FC.FREE_COUNTS)
def test_free_counts_around_the_wavefront_and_the_workgroup(F):
    _, kind, T0 = FC.counted(F)
    assert int((kind == FC.FREE).sum()) == F
    its = check_against_loop(fill_dev, ("counted", F), T0, kind, FC.SWEEPS_GPU)
    t, k = _dev(T0), _dev(kind)
    untouched = torch.from_numpy(np.broadcast_to(kind != FC.FREE, T0.shape).copy()).cuda()
    for n in FC.SWEEPS_GPU:
        first = FF.fill_device(t, k, n)
        again = FF.fill_device(t, k, n)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])       # the same bits on every run
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = FF.fill_device(t, k, n)
        side.synchronize()
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
        # FREE nodes lie on every face of the grid (F >= 6): whatever the list names, nothing outside the FREE nodes is written, in
        # either buffer -- every FIXED and OUT entry is the seed's
        for buf in first:
            assert same_bits(buf[untouched].cpu().numpy(), t[untouched].cpu().numpy())
        assert same_bits(first[0].cpu().numpy(), its[n])
    assert torch.equal(t, _dev(T0))                              # the input is left as it was


def test_analytic_line_on_the_device():
    field, kind = FC.line()
    res, prev = FF.fill_device(_dev(FF.seed(field, kind)), _dev(kind), FC.LINE_SWEEPS)
    d, conf = T.solve_device(FF.quantise_device(res), FC.LINE_SHAPE)
    FC.check_line(res.cpu().numpy(), d.cpu().numpy(), conf.cpu().numpy())
    host = FF.fill_numpy(FF.seed(field, kind), kind, FC.LINE_SWEEPS)
    assert same_bits(res.cpu().numpy(), host[0]) and same_bits(prev.cpu().numpy(), host[1])


@pytest.mark.parametrize("name", ("thirds", "borders"))
def test_quantise_solve_and_merge_agree_with_the_numpy_path(name):
    shape = FC.GRIDS["g1796"]
    dirs, kind, T0 = FC.pattern(name, shape)
    field = FC.field_of(dirs, kind, shape)
    res = FF.fill_numpy(T0, kind, 7)[0]
    acc = FF.quantise(res)
    acc_dev = FF.quantise_device(_dev(res))
    assert same_bits(acc_dev.cpu().numpy(), acc)
    d, conf = T.solve_device(acc_dev, shape)
    got, host = (d.cpu().numpy(), conf.cpu().numpy()), T.solve_numpy(acc)
    below, rows = TR.compare_solves(acc, got, host)
    assert rows > 300 and below <= 0.05 * rows
    merged = FF.merge(field, kind, *got)
    keep = kind != FC.FREE
    assert same_bits(merged.dir[keep], field.dir[keep]) and same_bits(merged.conf[keep], field.conf[keep])
    free = kind == FC.FREE
    assert same_bits(merged.dir[free], got[0][free]) and (merged.conf[free] >= 0).all() and (merged.conf[free] <= 1.0 + 1e-9).all()
    stats_d, stats_h = {}, {}
    whole = FF.fill_field(field, kind, 7, device="cuda", stats=stats_d)
    whole_h = FF.fill_field(field, kind, 7, stats=stats_h)
    assert same_bits(whole.dir, merged.dir) and same_bits(whole.conf, merged.conf) and stats_d["last_change"] == stats_h["last_change"]
    assert same_bits(whole_h.dir[keep], field.dir[keep]) and np.abs(whole_h.conf - whole.conf).max() <= 1e-9
    with pytest.raises(Exception, match="not finite"):
        bad = _dev(res)
        bad[2, 1, 1, 1] = float("nan")
        FF.quantise_device(bad)


def test_wrapper_refusals():
    import hgs_runtime as rt
    shape = FC.GRIDS["g543"]
    _, kind, T0 = FC.pattern("thirds", shape)
    t, k = _dev(T0), _dev(kind)
    index = torch.nonzero(k.reshape(-1) == FC.FREE).reshape(-1).to(torch.int32)
    a, b = t.clone(), t.clone()
    assert rt.fill_check(shape, k, a, b, index) == index.numel()
    bad_index = index.clone()
    bad_index[0] = 60
    low_index = index.clone()
    low_index[0] = -1
    for call in (lambda: FF.fill_device(t, k, -1),
                 lambda: FF.fill_device(t, k, 65537),
                 lambda: FF.fill_device(t.float(), k, 1),
                 lambda: FF.fill_device(t, k.to(torch.int32), 1),
                 lambda: FF.fill_device(t[:5].contiguous(), k, 1),
                 lambda: FF.fill_device(t, k[:-1].contiguous(), 1),
                 lambda: FF.fill_device(t.transpose(2, 3), k, 1),
                 lambda: rt.fill_check(shape, k, a, a, index),
                 lambda: rt.fill_check(shape, k, a, b[:5], index),
                 lambda: rt.fill_check((5, 4, 4), k, a, b, index),
                 lambda: rt.fill_check(shape, k, a, b, index.to(torch.int64)),
                 lambda: rt.fill_check(shape, k, a, b, bad_index),
                 lambda: rt.fill_check(shape, k, a, b, low_index),
                 lambda: rt.fill_check(shape, k, a, b, torch.zeros(61, dtype=torch.int32, device="cuda"))):
        with pytest.raises(rt.HgsError):
            call()


# ---- the driver --------------------------------------------------------------------------------------------------------------
def test_driver_fills_on_both_devices(tmp_path, capsys):
    import trace_strands as driver
    src = tmp_path / "scene"
    FC.write_scene(src)
    ply = lambda m: tmp_path / m / "point_cloud" / "iteration_1" / "point_cloud.ply"      # noqa: E731
    args = [a for a in DRIVER if a not in ("--device", "cpu")] + BOX
    n_cpu = driver.main(["-s", str(src), "-m", str(tmp_path / "cpu"), "--device", "cpu", "--field", str(tmp_path / "field.npz")] + args)
    counts_cpu = kind_counts(capsys.readouterr().out)
    n_cuda = driver.main(["-s", str(src), "-m", str(tmp_path / "cuda"), "--device", "cuda"] + args)
    counts_cuda = kind_counts(capsys.readouterr().out)
    assert counts_cuda == counts_cpu and n_cuda == n_cpu and n_cpu >= 0.9 * FC.ROOTS
    # fed the numpy path's filled volume, the kernel's trace writes the same bytes
    field = T.load_field(str(tmp_path / "field.npz"))
    plain = [a for a in DRIVER if a not in ("--device", "cpu")]
    assert driver.main(["-s", str(src), "-m", str(tmp_path / "cuda_given"), "--device", "cuda"] + plain, field=field) == n_cpu
    with open(ply("cpu"), "rb") as a, open(ply("cuda_given"), "rb") as b:
        assert a.read() == b.read()
