"""hgs_field_splat, hgs_field_solve and hgs_strand_trace (csrc/hgs_trace.hip) against the numpy paths of utils/trace.py and the loop
restatement of tests/trace_reference.py: the seven int64 sums bit for bit at point counts around the wavefront and the workgroup, on
the cubic and the two non-cubic grids, split and repeated; the Jacobi solve against numpy.linalg.eigh under
trace_reference.compare_solves; count, reason and every joint of the trace bit for bit; the refusals; the trace_strands.py driver on
both devices; and two training steps on the traced model."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import trace_cases as TC
from tests import trace_reference as TR
from tests.test_trace_cpu import DRIVER, SPLAT_CASES, _same, circle_case, solve_inputs, splat_case
from utils import trace as T

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- splat -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,n", SPLAT_CASES)
def test_splat_equals_the_restatement_and_the_numpy_path(grid, n):
    pts, dirs, want, skipped = splat_case(grid, n)
    shape = TC.GRIDS[grid]
    nx, ny, nz = shape
    p, d = _dev(pts), _dev(dirs)
    acc, sk = T.splat_device(p, d, TC.ORIGIN, TC.H, shape, TC.R)
    assert acc.dtype == torch.int64 and tuple(acc.shape) == (nz, ny, nx, 7) and sk.dtype == torch.int32
    assert acc.cpu().numpy().tobytes() == want.tobytes() and int(sk.cpu()[0]) == skipped
    host, host_skipped = T.splat_numpy(pts, dirs, TC.ORIGIN, TC.H, shape, TC.R)
    assert host.tobytes() == want.tobytes() and host_skipped == skipped
    again, _ = T.splat_device(p, d, TC.ORIGIN, TC.H, shape, TC.R)
    assert torch.equal(again, acc)                               # integer sums: the same bits on every launch
    n_pts = pts.shape[0]
    if n_pts >= 2:                                               # in two parts, reversed, on a side stream: the same bits
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            rp, rd = p.flip(0).contiguous(), d.flip(0).contiguous()
            part, sk2 = T.splat_device(rp[:n_pts // 3].contiguous(), rd[:n_pts // 3].contiguous(), TC.ORIGIN, TC.H, shape, TC.R)
            T.splat_device(rp[n_pts // 3:].contiguous(), rd[n_pts // 3:].contiguous(), TC.ORIGIN, TC.H, shape, TC.R, acc=part, skipped=sk2)
        side.synchronize()
        assert torch.equal(part, acc) and int(sk2.cpu()[0]) == skipped


def test_points_beyond_the_radius_touch_no_node():
    shape = TC.GRIDS["g543"]
    sp, sd, _ = TC.special_points(shape)
    for j in range(5, 5 + 36):
        out = (0.5 * TC.R, TC.R - 2.0 ** -30, TC.R, TC.R + 2.0 ** -30, 3.0 * TC.R, 40.0)[(j - 5) % 6]
        acc, _ = T.splat_device(_dev(sp[j:j + 1]), _dev(sd[j:j + 1]), TC.ORIGIN, TC.H, shape, TC.R)
        assert bool(acc.any()) == (out < TC.R), (j, out)
    far = np.array([[1e300, -1e300, 1e300], [1e18, 0.0, 0.0], [-1e18, 0.3, 1.1]])
    acc, sk = T.splat_device(_dev(far), _dev(np.ones((3, 3))), TC.ORIGIN, TC.H, shape, TC.R)
    assert not acc.any() and int(sk.cpu()[0]) == 0
    stats = {"acc": None}
    pts, dirs, want, skipped = splat_case("g1796", 257)
    f = T.build_field(pts, dirs, TC.ORIGIN, TC.H, TC.GRIDS["g1796"], TC.R, device="cuda", stats=stats)
    assert stats["acc"].tobytes() == want.tobytes() and stats["skipped"] == skipped and stats["nonempty"] == int((want[..., 0] != 0).sum())
    assert f.dir.shape == (6, 9, 17, 3) and f.conf.shape == (6, 9, 17)


# ---- solve -----------------------------------------------------------------------------------------------------------------
def test_solve_agrees_with_eigh():
    below = rows = 0
    combed, generic, hard = solve_inputs()
    for acc in (combed, generic):
        nz, ny, nx, _ = acc.shape
        host = T.solve_numpy(acc)
        d, conf = T.solve_device(_dev(acc), (nx, ny, nz))
        assert tuple(d.shape) == (nz, ny, nx, 3) and tuple(conf.shape) == (nz, ny, nx)
        got = (d.cpu().numpy(), conf.cpu().numpy())
        b, r = TR.compare_solves(acc, got, host)
        below, rows = below + b, rows + r
        d2, conf2 = T.solve_device(_dev(acc), (nx, ny, nz))
        assert torch.equal(d, d2) and torch.equal(conf, conf2)
    print(f"{below} of {rows} non-empty nodes below the gap")
    assert rows > 500 and below <= 0.05 * rows
    # the hard rows, as a 2 x 2 x 2 grid: empty, W == 0 with entries, isotropic, rank 1, a double top eigenvalue, huge, tiny, generic
    d, conf = (t.cpu().numpy().reshape(8, -1) for t in T.solve_device(_dev(hard.reshape(2, 2, 2, 7)), (2, 2, 2)))
    conf = conf.reshape(-1)
    hd, hc = T.solve_numpy(hard)
    norm = np.linalg.norm(d, axis=1)
    assert np.isfinite(d).all() and np.isfinite(conf).all()
    assert norm[0] == 0 and norm[1] == 0 and conf[0] == 0 and conf[1] == 0
    assert np.allclose(norm[2:], 1.0, rtol=0, atol=1e-12)
    assert conf[2] == 0 and abs(conf[3] - 1.0) < 1e-9 and np.abs(d[3] - [0.6, 0.0, 0.8]).max() < 1e-9
    assert conf[4] == 0 and abs(d[4, 2]) < 1e-12
    below, rows = TR.compare_solves(hard, (d, conf), (hd, hc))   # the same rule, whatever the scale (huge: 2^24, tiny: 2^-32)
    assert (below, rows) == (2, 6)                               # the isotropic row and the double eigenvalue have no gap


# ---- trace -----------------------------------------------------------------------------------------------------------------
def _trace_dev(roots, p0, field, **knobs):
    kn = dict(TC.KNOBS, **knobs)
    out = T.trace_device(_dev(roots), _dev(p0), _dev(field.dir), _dev(field.conf), field.origin, field.spacing, field.shape, **kn)
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("S", TC.SS)
def test_trace_equals_the_restatement_on_the_circular_field(S):
    roots, p0, want = circle_case()
    f = TC.circular_field()
    got = _trace_dev(roots[:S], p0[:S], f)
    assert got[0].shape == (S, TC.KNOBS["max_steps"] + 1, 3) and got[1].dtype == np.int32 and got[2].dtype == np.int32
    _same(got, tuple(w[:S] for w in want))
    _same(got, T.trace_numpy(roots[:S], p0[:S], f, **TC.KNOBS))
    _same(_trace_dev(roots[:S], p0[:S], TC.circular_field(flip=True)), got)      # half of the dir entries negated: equal bits
    if S == max(TC.SS):
        _same(T.trace(roots, p0, f, device="cuda", budget=24 * (TC.KNOBS["max_steps"] + 1) * 70, **TC.KNOBS), got)   # five batches


def test_stop_reasons_on_the_device():
    mid = (3.5, 2.5)
    root, p0 = TC.at(1.0, *mid)[None], np.array([[1.0, 0.0, 0.0]])
    cases = [(root, p0, TC.half_spaces(), dict(cos_max=np.cos(np.radians(30.0))), T.TURN, None),
             (root, p0, TC.half_spaces(), dict(), T.BOUNDS, None),
             (root, p0, TC.slab_field(4, 5), dict(max_gap=3, max_steps=100), T.BOUNDS, 31),
             (root, p0, TC.slab_field(4, 5), dict(max_gap=2, max_steps=100), T.GAP, 7),
             (TC.at(TC.CENTRE[0], TC.CENTRE[1], 2.5)[None], np.array([[0.8, 0.6, 0.0]]), TC.circular_field(core=1.6), dict(max_gap=6), None, None),
             (TC.at(TC.CENTRE[0], TC.CENTRE[1], 2.5)[None], np.array([[0.8, 0.6, 0.0]]), TC.circular_field(core=1.6), dict(max_gap=1), T.GAP, 1),
             (root, p0, TC.uniform_field(), dict(max_steps=3), T.STEPS, 4),
             (root, p0, TC.uniform_field(), dict(max_steps=1), T.STEPS, 2),
             (root, p0, TC.uniform_field(), dict(max_steps=200), T.BOUNDS, 31),
             (root, p0, TC.uniform_field(d=(0.5, 0.3, -0.2)), dict(max_steps=200), T.BOUNDS, None),
             (np.array([[np.nan, 0.0, 0.0], TC.at(-1.0, 1.0, 1.0), TC.at(3.0, 3.0, 5.0)]), np.tile(p0, (3, 1)), TC.uniform_field(), dict(), T.BOUNDS, 1)]
    for r, p, f, knobs, reason, count in cases:
        kn = dict(TC.KNOBS, **knobs)
        got = _trace_dev(r, p, f, **knobs)
        _same(got, TR.trace(r, p, f.origin, f.spacing, f.shape, f.dir, f.conf, **kn))
        _same(got, T.trace_numpy(r, p, f, **kn))
        if reason is not None:
            assert (got[2] == reason).all(), (knobs, got[2])
        else:
            assert got[1][0] > 12 and got[2][0] != T.GAP          # from the empty core into the field, and on
        if count is not None:
            assert (got[1] == count).all(), (knobs, got[1])
    joints, count, reason = _trace_dev(root, p0, TC.uniform_field(), max_steps=200)
    x = root[0].copy()
    for j in range(1, count[0]):
        x = x + TC.STEP * np.array([1.0, 0.0, 0.0])
        assert joints[0, j].tobytes() == x.tobytes()             # the sequential sums' bits


def test_wrapper_refusals():
    import hgs_runtime as rt
    f = TC.uniform_field()
    pts, dirs = TC.cloud(TC.GRIDS["g543"], 8)
    p, d = _dev(pts), _dev(dirs)
    shape = TC.GRIDS["g543"]
    for call in (lambda: T.splat_device(p.float(), d, TC.ORIGIN, TC.H, shape, TC.R),
                 lambda: T.splat_device(p, d[:4].contiguous(), TC.ORIGIN, TC.H, shape, TC.R),
                 lambda: T.splat_device(p, d, TC.ORIGIN, TC.H, shape, 9.0 * TC.H),
                 lambda: T.splat_device(p, d, TC.ORIGIN, 0.0, shape, TC.R),
                 lambda: T.splat_device(p, d, TC.ORIGIN, TC.H, shape, TC.R, acc=torch.zeros((3, 4, 4, 7), dtype=torch.int64, device="cuda")),
                 lambda: T.splat_device(p, d, TC.ORIGIN, TC.H, shape, TC.R, acc=torch.zeros((3, 4, 5, 7), dtype=torch.int32, device="cuda")),
                 lambda: T.splat_device(p, d, TC.ORIGIN, TC.H, shape, TC.R, skipped=torch.zeros(2, dtype=torch.int32, device="cuda")),
                 lambda: T.solve_device(torch.zeros((3, 4, 5, 7), dtype=torch.int64, device="cuda"), (5, 4, 4)),
                 lambda: T.solve_device(torch.zeros((3, 4, 5, 7), dtype=torch.float64, device="cuda"), shape),
                 lambda: _trace_dev(pts, dirs, T.Field(f.origin, f.spacing, f.shape, f.dir, f.conf), max_steps=0),
                 lambda: T.trace_device(p, d, _dev(f.dir)[:-1].contiguous(), _dev(f.conf), f.origin, f.spacing, f.shape, **TC.KNOBS),
                 lambda: T.trace_device(p, d, _dev(f.dir), _dev(f.conf).float(), f.origin, f.spacing, f.shape, **TC.KNOBS),
                 lambda: T.trace_device(p, d, _dev(f.dir), _dev(f.conf), f.origin, f.spacing, (17, 9, 7), **TC.KNOBS)):
        with pytest.raises(rt.HgsError):
            call()


# ---- the driver --------------------------------------------------------------------------------------------------------------
def _joints(ply):
    from utils.ply import read_ply
    v = dict(read_ply(str(ply)))["vertex"]
    return np.stack([np.asarray(v[n], np.float32) for n in "xyz"], axis=1)


def test_driver_on_both_devices(tmp_path, capsys):
    import trace_strands as driver
    src = tmp_path / "scene"
    pts, normals = TC.write_scene(src)
    ply = lambda m: tmp_path / m / "point_cloud" / "iteration_1" / "point_cloud.ply"      # noqa: E731
    args = [a for a in DRIVER if a not in ("--device", "cpu")]
    n_cpu = driver.main(["-s", str(src), "-m", str(tmp_path / "cpu"), "--device", "cpu", "--field", str(tmp_path / "field.npz")] + args)
    field = T.load_field(str(tmp_path / "field.npz"))
    # fed the numpy field, the kernel's trace writes the same bytes
    assert driver.main(["-s", str(src), "-m", str(tmp_path / "cuda_given"), "--device", "cuda"] + args, field=field) == n_cpu
    with open(ply("cpu"), "rb") as a, open(ply("cuda_given"), "rb") as b:
        assert a.read() == b.read()
    # with the device's own field: the two fields differ by the solvers' 1e-12 (about 1e-9 rad at the gap floor, and a node near
    # the floor carries next to no aligned mass), a joint after 60 steps by far less than half a float32 ulp: the stored float32
    # coordinates differ by one ulp of the scene's largest coordinate at the very most, on a rounding boundary
    n_cuda = driver.main(["-s", str(src), "-m", str(tmp_path / "cuda"), "--device", "cuda"] + args)
    out = capsys.readouterr().out
    assert n_cuda == n_cpu and out.count("stopped by gap") == 3
    a, b = _joints(ply("cpu")), _joints(ply("cuda"))
    ulp = float(np.spacing(np.float32(np.abs(a).max())))
    worst = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    print(f"{n_cpu} strands, {a.shape[0]} joints: largest difference {worst:.3e}, one float32 ulp of the scene {ulp:.3e}, {int((a != b).sum())} values differ")
    assert a.shape == b.shape == (12 * n_cpu, 3) and worst <= ulp


def test_traced_model_takes_training_steps(tmp_path):
    import trace_strands as driver
    from arguments import OptimizationParams
    from scene import Scene
    from scene.hair_gaussian_model import HairGaussianModel
    from train import training_step
    src, model = tmp_path / "scene", tmp_path / "model"
    TC.write_scene(src)
    n = driver.main(["-s", str(src), "-m", str(model), "--device", "cuda"] + [a for a in DRIVER if a not in ("--device", "cpu")])
    args = SimpleNamespace(source_path=str(src), model_path=str(model), images="images", sh_degree=0, resolution=-1, data_device="cuda", eval=False)
    scene = Scene(args, shuffle=False)
    g = scene.gaussians
    assert isinstance(g, HairGaussianModel) and len(g.strands_info.offsets) - 1 == n and g._endpoints.shape[0] == 12 * n
    opt = OptimizationParams()
    opt.enable_topology = False
    g.training_setup(opt)
    before = g._endpoints.detach().clone()
    cams = scene.getCameras()
    assert len(cams) == 2 and cams[0].image_height == 64 and cams[0].image_width == 64
    for it, cam in enumerate(cams, 1):
        loss = training_step(g, cam, opt, torch.zeros(3, device="cuda"), it, extent=scene.cameras_extent)[0]
        assert np.isfinite(float(loss))
    assert torch.isfinite(g._endpoints).all() and not torch.equal(before, g._endpoints.detach())
