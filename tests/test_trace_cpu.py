"""The direction volume and the strand trace without a GPU: the numpy paths of utils/trace.py against the loop restatement of
tests/trace_reference.py (the int64 sums and every traced joint bit for bit), the eigh solve's own margins on the chosen inputs, the
trace's stop reasons on hand-made fields, the entry points' refusals and the trace_strands.py driver on a synthetic scene."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import trace_cases as TC
from tests import trace_reference as TR
from utils import trace as T

_SPLATS = {}


def splat_case(grid, n):
    """(points, dirs, reference sums, reference skipped) of a cloud case, computed once and left unchanged."""
    key = (grid, n)
    if key not in _SPLATS:
        shape = TC.GRIDS[grid]
        pts, dirs = TC.pile(shape) if n == "pile" else TC.cloud(shape, n)
        acc, skipped = TR.splat(pts, dirs, TC.ORIGIN, TC.H, shape, TC.R)
        acc.setflags(write=False)
        _SPLATS[key] = (pts, dirs, acc, skipped)
    return _SPLATS[key]


SPLAT_CASES = [(g, n) for g in TC.GRIDS for n in TC.NS] + [("g543", "pile")]


@pytest.mark.parametrize("grid,n", SPLAT_CASES)
def test_numpy_splat_equals_the_restatement(grid, n):
    pts, dirs, want, skipped = splat_case(grid, n)
    shape = TC.GRIDS[grid]
    acc, got_skipped = T.splat_numpy(pts, dirs, TC.ORIGIN, TC.H, shape, TC.R)
    nx, ny, nz = shape
    assert acc.dtype == np.int64 and acc.shape == (nz, ny, nx, 7)
    assert acc.tobytes() == want.tobytes() and got_skipped == skipped
    if n != "pile" and n >= 2:                                   # in two parts, added to one array: the same bits
        part, s1 = T.splat_numpy(pts[:n // 2], dirs[:n // 2], TC.ORIGIN, TC.H, shape, TC.R)
        part, s2 = T.splat_numpy(pts[n // 2:], dirs[n // 2:], TC.ORIGIN, TC.H, shape, TC.R, acc=part)
        assert part.tobytes() == want.tobytes() and s1 + s2 == skipped


def test_the_special_points_are_what_they_claim():
    shape = TC.GRIDS["g543"]
    sp, sd, n_skipped = TC.special_points(shape)
    acc, skipped = TR.splat(sp, sd, TC.ORIGIN, TC.H, shape, TC.R)
    assert skipped == n_skipped
    one = 1 << 32
    # a point on a node gives it k == 1: the far corner holds exactly one such point and nothing else within r
    assert acc[2, 3, 4, 0] == one
    # the point at d2 == r2 from node (1, 1, 1) is excluded there: alone, it reaches nodes of ix = 2 and 3 only (ix = 1 and 4 are r away
    # along x at the least)
    alone, _ = TR.splat(sp[4:5], sd[4:5], TC.ORIGIN, TC.H, shape, TC.R)
    assert alone[1, 1, 1, 0] == 0 and alone[1, 1, 2, 0] > 0 and alone[1, 1, 3, 0] > 0 and not alone[:, :, [0, 1, 4]].any()
    assert alone[1, 1, 2, 4] > 0 and not alone[1, 1, 2, [1, 2, 3, 5, 6]].any()                 # its direction is +y: yy alone
    # outside a face by r or more: no node; by less: some node
    for j in range(5, 5 + 36):
        out = (0.5 * TC.R, TC.R - 2.0 ** -30, TC.R, TC.R + 2.0 ** -30, 3.0 * TC.R, 40.0)[(j - 5) % 6]
        a, _ = TR.splat(sp[j:j + 1], sd[j:j + 1], TC.ORIGIN, TC.H, shape, TC.R)
        assert bool(a.any()) == (out < TC.R), (j, out)
    pile = splat_case("g543", "pile")
    assert (pile[2][1, 2, 2, 0] > 100 * one) and pile[3] == 0                                  # 300 points on one node
    # the trace of T is W up to the roundings of the seven terms: 3.5 units a point at the very most
    W, tr = acc[..., 0], acc[..., 1] + acc[..., 4] + acc[..., 6]
    assert np.abs(W - tr).max() <= 4 * sp.shape[0]


def test_splat_refusals():
    shape = TC.GRIDS["g543"]
    pts, dirs = TC.cloud(shape, 8)
    for kw in (dict(shape=(1, 4, 4)), dict(shape=(4, 1025, 4)), dict(shape=(1024, 1024, 128)), dict(h=0.0), dict(h=float("nan")),
               dict(origin=(0.0, np.inf, 0.0)), dict(r=0.0), dict(r=float("nan")), dict(r=8.5 * TC.H), dict(dirs=dirs[:4]),
               dict(points=pts[:, :2])):
        a = dict(points=pts, dirs=dirs, origin=TC.ORIGIN, h=TC.H, shape=shape, r=TC.R)
        a.update(kw)
        with pytest.raises(ValueError):
            T.splat_numpy(**a)
    with pytest.raises(ValueError):
        T.splat_numpy(pts, dirs, TC.ORIGIN, TC.H, shape, TC.R, acc=np.zeros((3, 4, 5, 7), np.int32))


# ---- solve -----------------------------------------------------------------------------------------------------------------
def solve_inputs():
    """The sums the solve tests use: a combed cloud on the 17 x 9 x 6 grid, the generic cloud on it, and the hard rows."""
    shape = TC.GRIDS["g1796"]
    pts, dirs = TC.combed(shape, 4000)
    return [T.splat_numpy(pts, dirs, TC.ORIGIN, TC.H, shape, TC.R)[0], splat_case("g1796", 257)[2].copy(), TC.hard_sums()]


def test_host_solve_stays_within_its_margins():
    """The eigh path alone: unit vectors, the sign rule, zero rows where W == 0, and no more than 5 % of the non-empty nodes of the
    chosen inputs below the relative eigen-gap of 1e-6 that the device comparison leaves out."""
    below = rows = 0
    for acc in solve_inputs()[:2]:
        host = T.solve_numpy(acc)
        assert host[0].shape == acc.shape[:-1] + (3,) and host[1].shape == acc.shape[:-1]
        b, r = TR.compare_solves(acc, host, host)
        below, rows = below + b, rows + r
        conf, W = host[1].reshape(-1), acc.reshape(-1, 7)[:, 0] / 4294967296.0
        assert (conf >= 0).all() and (conf <= W + 1e-6).all()                                  # the aligned mass is part of the mass
    assert rows > 500 and below <= 0.05 * rows, (below, rows)
    hard = TC.hard_sums()
    d, conf = T.solve_numpy(hard)
    norm = np.linalg.norm(d, axis=1)
    assert norm[0] == 0 and norm[1] == 0 and conf[0] == 0 and conf[1] == 0
    assert np.allclose(norm[2:], 1.0, rtol=0, atol=1e-12)
    assert conf[2] == 0 and abs(conf[3] - 1.0) < 1e-9 and np.abs(np.abs(d[3]) - [0.6, 0.0, 0.8]).max() < 1e-9 and d[3, 2] > 0
    assert conf[4] == 0 and abs(d[4, 2]) < 1e-12                                               # the top eigenvalue is double: in the xy plane
    assert conf[5] > 2.0 ** 20 and 0 < conf[6] < 2.0 ** -30                                      # huge and tiny entries
    with pytest.raises(ValueError):
        T.solve_numpy(hard.astype(np.float64))


# ---- trace -----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """count, reason and every joint below count: equal bits."""
    (ja, ca, ra), (jb, cb, rb) = a, b
    assert ca.dtype == cb.dtype == np.int32 and ra.dtype == rb.dtype == np.int32
    assert np.array_equal(ca, cb) and np.array_equal(ra, rb)
    live = np.arange(ja.shape[1])[None, :] < ca[:, None]
    assert ja.shape == jb.shape and ja[live].tobytes() == jb[live].tobytes()


def _both(roots, p0, field, **knobs):
    kn = dict(TC.KNOBS, **knobs)
    got = T.trace_numpy(roots, p0, field, **kn)
    want = TR.trace(roots, p0, field.origin, field.spacing, field.shape, field.dir, field.conf, **kn)
    _same(got, want)
    return got


_CIRCLE = {}


def circle_case():
    """(roots, p0, the reference's result) on the circular field, computed once."""
    if not _CIRCLE:
        f = TC.circular_field()
        roots, p0 = TC.roots(max(TC.SS))
        _CIRCLE["v"] = (roots, p0, TR.trace(roots, p0, f.origin, f.spacing, f.shape, f.dir, f.conf, **TC.KNOBS))
    return _CIRCLE["v"]


@pytest.mark.parametrize("S", TC.SS)
def test_numpy_trace_equals_the_restatement_on_the_circular_field(S):
    roots, p0, want = circle_case()
    f = TC.circular_field()
    got = T.trace_numpy(roots[:S], p0[:S], f, **TC.KNOBS)
    _same(got, tuple(w[:S] for w in want))
    assert got[0].shape == (S, TC.KNOBS["max_steps"] + 1, 3)
    flipped = T.trace_numpy(roots[:S], p0[:S], TC.circular_field(flip=True), **TC.KNOBS)
    _same(flipped, got)                                          # half of the dir entries negated: equal bits
    if S == max(TC.SS):
        joints, count, reason = got
        assert set(np.unique(reason)) >= {T.STEPS, T.BOUNDS, T.TURN}         # (GAP: test_stop_reasons)
        special = [0, 1, 2, 3, 4, 6, 7]                          # NaN, outside, t == n - 1 on each axis, overflow, infinity
        assert (count[special] == 1).all() and (reason[special] == T.BOUNDS).all()
        assert count.max() > 20
        # batched by a budget of a few roots: the same result
        small = T.trace(roots, p0, f, device=None, budget=24 * (TC.KNOBS["max_steps"] + 1) * 7, **TC.KNOBS)
        _same(small, got)
        assert T.batch_roots(48, 24 * 49 * 7) == 7 and T.batch_roots(4096, 1) == 1


def test_uniform_field_steps_are_sequential_sums():
    f = TC.uniform_field()
    roots = np.array([TC.at(1.0, 3.5, 2.5), TC.at(0.3, 0.7, 0.2), TC.at(15.9, 7.9, 4.9)])
    p0 = np.array([[1.0, 0.0, 0.0], [0.6, 0.0, 0.8], [0.0, -1.0, 0.0]])
    joints, count, reason = _both(roots, p0, f, max_steps=200)
    assert (reason == T.BOUNDS).all()
    for s in range(3):
        x = roots[s].copy()
        for j in range(1, count[s]):
            x = x + TC.STEP * np.array([1.0, 0.0, 0.0])          # d = v / sqrt(dot(v, v)) is (1, 0, 0) exactly for v = (w, 0, 0)
            assert joints[s, j].tobytes() == x.tobytes()
        t_last = (joints[s, count[s] - 1, 0] - TC.ORIGIN[0]) / TC.H
        assert t_last >= 16.0 and t_last - 0.5 < 16.0            # the far face: the first joint at or past the last node
    generic = TC.uniform_field(d=(0.5, 0.3, -0.2))
    j2, c2, r2 = _both(roots, p0, generic, max_steps=200)
    assert (r2 == T.BOUNDS).all() and (c2 > 1).all()
    d = np.array([0.5, 0.3, -0.2]) / np.linalg.norm([0.5, 0.3, -0.2])
    line = j2[0, 1:c2[0]] - roots[0]
    assert np.abs(np.cross(line, d)).max() < 1e-12


def test_stop_reasons():
    mid = (3.5, 2.5)
    # two half-spaces 90 degrees apart: the interpolated direction turns by 45 degrees a half-voxel step
    joints, count, reason = _both(TC.at(1.0, *mid)[None], np.array([[1.0, 0.0, 0.0]]), TC.half_spaces(), cos_max=np.cos(np.radians(30.0)))
    assert reason[0] == T.TURN and 10 <= count[0] <= 16
    _, count60, reason60 = _both(TC.at(1.0, *mid)[None], np.array([[1.0, 0.0, 0.0]]), TC.half_spaces(), cos_max=0.5)
    assert reason60[0] == T.BOUNDS and count60[0] > count[0]     # at 60 degrees the same strand makes the turn
    # an empty slab: conf 0 at ix = 4, 5.  From t = 1 in steps of 0.5: w = 1, .., 1, 0.5 (t = 3.5: still >= min_conf), then 0 at
    # t = 4, 4.5, 5 and 0.5 at t = 5.5: three steps coast
    root, p0 = TC.at(1.0, *mid)[None], np.array([[1.0, 0.0, 0.0]])
    slab = TC.slab_field(4, 5)
    joints, count, reason = _both(root, p0, slab, max_gap=3, max_steps=100)
    assert reason[0] == T.BOUNDS and count[0] == 31              # bridged: t = 1, 1.5, .., 16
    joints, count, reason = _both(root, p0, slab, max_gap=2, max_steps=100)
    assert reason[0] == T.GAP and count[0] == 7                  # the joints at t = 4.5 and 5 coasted: cut back to t = 4
    assert joints[0, 6].tobytes() == TC.at(4.0, *mid).tobytes()
    # a root in the empty core, p0 radial: it coasts to the field and enters it without a turn stop, tangentially
    core = TC.circular_field(core=1.6)
    c = TC.at(TC.CENTRE[0], TC.CENTRE[1], 2.5)
    p_rad = np.array([[0.8, 0.6, 0.0]])
    joints, count, reason = _both(c[None], p_rad, core, max_gap=6)
    assert count[0] > 12 and reason[0] != T.GAP
    want = TR.trace(c[None], p_rad, core.origin, core.spacing, core.shape, core.dir, core.conf, **dict(TC.KNOBS, max_gap=6))
    rad = np.linalg.norm((joints[0, :count[0], :2] - c[:2]) / TC.H, axis=1)
    assert rad[count[0] - 1] > 1.6 and np.array_equal(want[1], count)
    _, count_short, reason_short = _both(c[None], p_rad, core, max_gap=1)
    assert reason_short[0] == T.GAP and count_short[0] == 1      # too short a reach: nothing but the root is left
    # max_steps
    joints, count, reason = _both(TC.at(1.0, *mid)[None], p0, TC.uniform_field(), max_steps=3)
    assert reason[0] == T.STEPS and count[0] == 4 and joints.shape == (1, 4, 3)
    # a NaN root, a root outside
    bad = np.array([[np.nan, 0.0, 0.0], TC.at(-1.0, 1.0, 1.0), TC.at(3.0, 3.0, 5.0)])
    joints, count, reason = _both(bad, np.tile(p0, (3, 1)), TC.uniform_field())
    assert (count == 1).all() and (reason == T.BOUNDS).all()
    # no roots
    joints, count, reason = _both(np.zeros((0, 3)), np.zeros((0, 3)), TC.uniform_field())
    assert joints.shape == (0, 49, 3) and count.shape == (0,)


def test_trace_refusals_and_helpers():
    f = TC.uniform_field()
    r, p = TC.roots(4)
    for kw in (dict(max_steps=0), dict(max_steps=4097), dict(step=0.0), dict(step=float("nan")), dict(cos_max=1.5), dict(cos_max=float("nan")),
               dict(min_conf=float("inf")), dict(max_gap=-1)):
        with pytest.raises(ValueError):
            T.trace_numpy(r, p, f, **dict(TC.KNOBS, **kw))
    with pytest.raises(ValueError):
        T.trace_numpy(r, p[:2], f, **TC.KNOBS)
    with pytest.raises(ValueError):
        T.Field(TC.ORIGIN, TC.H, (5, 4, 3), np.zeros((3, 4, 5, 3)), np.zeros((3, 4, 4)))
    # resampling: a straight strand of 5 joints to 9; a bent one keeps its ends and its length
    J = np.zeros((2, 6, 3))
    J[0, :5, 0] = np.arange(5)
    J[1, :4] = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 2]]
    out = T.resample(J, np.array([5, 4]), 9)
    assert np.allclose(out[0, :, 0], np.arange(9) * 0.5) and not out[0, :, 1:].any()
    assert out[1, 0].tolist() == [0, 0, 0] and out[1, -1].tolist() == [1, 1, 2]
    assert np.allclose(T.lengths(J, np.array([5, 4])), [4.0, 4.0]) and np.allclose(T.lengths(out, np.array([9, 9])), [4.0, 4.0])
    assert np.allclose(np.linalg.norm(np.diff(out[1], axis=0), axis=1).sum(), 4.0)
    with pytest.raises(ValueError):
        T.resample(J, np.array([5, 1]), 9)
    p0 = T.initial_directions(np.array([[0.0, 0.0, 2.0], [1.0, 1.0, 1.0]]), np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 2.0]]))
    assert np.allclose(p0[0], np.array([-1.0, -1.0, 1.0]) / np.sqrt(3.0)) and p0[1].tolist() == [0.0, 0.0, 1.0]
    origin, h, shape = T.grid_box(np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.5]]), np.array([[1.0, 1.0, 1.0]]), 32, 1.5)
    assert shape[0] in (32, 33) and shape[1] < shape[0] and np.allclose(origin, -3 * h) and abs(h - 2.0 / 25) < 1e-12
    with pytest.raises(ValueError):
        T.grid_box(np.zeros((2, 3)), np.zeros((1, 3)), 32, 1.5)


def test_field_file_and_head_exclusion(tmp_path):
    from tests import head_sdf_cases as HC
    f = TC.circular_field()
    path = str(tmp_path / "field.npz")
    T.save_field(path, f)
    back = T.load_field(path)
    assert back.shape == f.shape and back.dir.tobytes() == f.dir.tobytes() and back.conf.tobytes() == f.conf.tobytes()
    np.savez(path, origin=f.origin)
    with pytest.raises(ValueError, match="direction volume"):
        T.load_field(path)
    sdf = HC.ball_field()
    nx, ny, nz = sdf.shape
    g = T.Field(sdf.origin, sdf.spacing, sdf.shape, np.zeros((nz, ny, nx, 3)), np.ones((nz, ny, nx)))
    cleared = T.exclude_head(g, sdf, 0.0)
    assert cleared == int((sdf.phi < 0).sum()) and np.array_equal(g.conf == 0, sdf.phi < 0)      # at the nodes the sample is phi itself
    more = T.exclude_head(g, sdf, 0.1)
    want = sdf.phi < 0.1
    want[-1], want[:, -1], want[:, :, -1] = False, False, False  # (t == n - 1 is out of the sample's range: outside the head)
    assert more > 0 and np.array_equal(g.conf == 0, want)


# ---- binding ---------------------------------------------------------------------------------------------------------------
def test_binding_symbols_and_refusals():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    for name, n_args in {"hgs_field_splat": 14, "hgs_field_solve": 7, "hgs_strand_trace": 21}.items():
        assert hasattr(L, name) and len(rt.SIGNATURES[name][1]) == n_args
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                    # (never dereferenced: every call below is refused first)

    def splat(N=4, pts=p, dirs=p, o=(0.0, 0.0, 0.0), h=0.25, n=(4, 4, 4), r2=0.1, acc=p, skipped=p):
        assert L.hgs_field_splat(None, N, pts, dirs, o[0], o[1], o[2], h, n[0], n[1], n[2], r2, acc, skipped) != 0
        return L.hgs_last_error().decode()

    def solve(n=(4, 4, 4), acc=p, d=p, conf=p):
        assert L.hgs_field_solve(None, n[0], n[1], n[2], acc, d, conf) != 0
        return L.hgs_last_error().decode()

    def trace(S=4, roots=p, p0=p, d=p, conf=p, o=(0.0, 0.0, 0.0), h=0.25, n=(4, 4, 4), step=0.1, max_steps=8, cos_max=0.5, min_conf=0.5,
              max_gap=2, joints=p, count=p, reason=p):
        assert L.hgs_strand_trace(None, S, roots, p0, d, conf, o[0], o[1], o[2], h, n[0], n[1], n[2], step, max_steps, cos_max, min_conf,
                                  max_gap, joints, count, reason) != 0
        return L.hgs_last_error().decode()
    inf, nan = float("inf"), float("nan")
    for N in (-1, (1 << 24) + 1):
        assert splat(N=N).startswith("hgs_field_splat: ") and "points" in splat(N=N)
    for n in ((1, 4, 4), (4, 1025, 4), (4, 4, 0), (1024, 1024, 65)):
        assert "a grid of" in splat(n=n) and "a grid of" in solve(n=n) and "a grid of" in trace(n=n)
    for h in (0.0, -1.0, inf, nan, 1e-320):
        assert "spacing" in splat(h=h) and "spacing" in trace(h=h)
    assert "origin" in splat(o=(nan, 0.0, 0.0)) and "origin" in trace(o=(0.0, inf, 0.0))
    for r2 in (0.0, -1.0, inf, nan, 4.1):                        # (4.1: a radius of more than 8 spacings of 0.25)
        assert "r2" in splat(r2=r2)
    for kw in (dict(pts=None), dict(dirs=None), dict(acc=None), dict(skipped=None)):
        assert splat(**kw).endswith("are required")
    for kw in (dict(acc=None), dict(d=None), dict(conf=None)):
        assert solve(**kw).startswith("hgs_field_solve: ") and solve(**kw).endswith("are required")
    assert "roots" in trace(S=-1) and "roots" in trace(S=(1 << 24) + 1)
    for ms in (0, -1, 4097):
        assert "max_steps" in trace(max_steps=ms)
    for kw in (dict(step=0.0), dict(step=nan), dict(step=inf), dict(cos_max=nan), dict(cos_max=1.5), dict(min_conf=nan), dict(max_gap=-1)):
        assert trace(**kw).startswith("hgs_strand_trace: step")
    for kw in (dict(roots=None), dict(p0=None), dict(d=None), dict(conf=None), dict(joints=None), dict(count=None), dict(reason=None)):
        assert trace(**kw).endswith("are required")
    assert L.hgs_field_splat(None, 0, None, None, 0.0, 0.0, 0.0, 0.25, 4, 4, 4, 0.1, p, p) == 0     # N == 0 launches nothing
    assert L.hgs_strand_trace(None, 0, None, None, p, p, 0.0, 0.0, 0.0, 0.25, 4, 4, 4, 0.1, 8, 0.5, 0.5, 2, None, None, None) == 0
    import torch
    with pytest.raises(rt.HgsError):
        T.splat_device(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), TC.ORIGIN, TC.H, (4, 4, 4), TC.R)
    with pytest.raises(rt.HgsError):
        T.solve_device(torch.zeros(4, 4, 4, 7, dtype=torch.int64), (4, 4, 4))                     # CPU tensors: the kernels have no CPU path
    f = TC.uniform_field()
    with pytest.raises(rt.HgsError):
        T.trace_device(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), torch.from_numpy(f.dir),
                       torch.from_numpy(f.conf), f.origin, f.spacing, f.shape, **TC.KNOBS)


# ---- the driver --------------------------------------------------------------------------------------------------------------
DRIVER = ["--device", "cpu", "--grid", "28", "--points", "12", "--max_steps", "60"]


def test_driver_on_cpu(tmp_path, capsys):
    import trace_strands as driver
    from utils.ply import read_ply
    src, model = tmp_path / "scene", tmp_path / "model"
    TC.write_scene(src)
    n = driver.main(["-s", str(src), "-m", str(model), "--field", str(tmp_path / "field.npz")] + DRIVER)
    out = capsys.readouterr().out
    assert n > 30 and f"{n} strand(s) kept" in out and "skipped" in out and "not empty" in out and "stopped by gap" in out
    assert f"{n} strand(s) of 12 joints written" in out
    ply = model / "point_cloud" / "iteration_1" / "point_cloud.ply"
    els = read_ply(str(ply))
    assert len(els) == 5 and dict(els)["vertex"]["x"].shape[0] == 12 * n
    assert os.path.exists(model / "input.ply") and os.path.exists(model / "cameras.json")
    with open(model / "input.ply", "rb") as a, open(src / "sparse" / "0" / "points3D.ply", "rb") as b:
        assert a.read() == b.read()
    field = T.load_field(str(tmp_path / "field.npz"))
    assert max(field.shape) in (28, 29) and (field.conf > 0.5).any()
    # what Scene makes of it: a strand model of n strands with 12 joints each
    from scene import Scene
    from scene.hair_gaussian_model import HairGaussianModel
    args = SimpleNamespace(source_path=str(src), model_path=str(model), images="images", sh_degree=0, resolution=-1, data_device="cpu", eval=False)
    scene = Scene(args, shuffle=False)
    g = scene.gaussians
    assert isinstance(g, HairGaussianModel) and scene.loaded_iter == 1
    off = np.asarray(g.strands_info.offsets)
    assert len(off) - 1 == n and (np.diff(off) == 11).all()      # 11 segments: 12 joints
    # the strands start on the scalp and have uniform segments, 4 joints of half a voxel at the least before the resampling
    ep = g._endpoints.detach().numpy().reshape(n, 12, 3).astype(np.float64)
    assert np.abs(np.linalg.norm(ep[:, 0], axis=1) - 0.5).max() < 1e-6
    seg = np.linalg.norm(np.diff(ep, axis=1), axis=2)
    assert (seg.sum(axis=1) >= 3 * 0.5 * field.spacing * (1 - 1e-6)).all() and (seg.max(axis=1) - seg.min(axis=1) <= 0.2 * seg.max(axis=1)).all()
    # a given field is traced as it is: the same bytes again
    with open(ply, "rb") as fh:
        first = fh.read()
    assert driver.main(["-s", str(src), "-m", str(model), "--overwrite"] + DRIVER, field=field) == n
    with open(ply, "rb") as fh:
        assert fh.read() == first
    assert driver.main(["-s", str(src), "-m", str(tmp_path / "few"), "--roots", "10", "--min_joints", "2"] + DRIVER) <= 10


def test_driver_refusals(tmp_path):
    import trace_strands as driver
    src = tmp_path / "scene"
    TC.write_scene(src, n_points=500, directions=False, head=False)
    run = lambda *extra: driver.main(["-s", str(src), "-m", str(tmp_path / "model")] + DRIVER + list(extra))     # noqa: E731
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: .*no non-zero normal.*init_cloud\.py --directions"):
        run()
    os.remove(src / "sparse" / "0" / "points3D.ply")
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: .*points3D\.ply is missing.*init_cloud\.py --directions"):
        run()
    TC.write_scene(src, n_points=3000, head=False)
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: .*head_reconstruction_data\.npz is missing.*init_scalp\.py"):
        run()
    assert not os.path.exists(tmp_path / "model")                # (refused before anything is written)
    TC.write_scene(src, n_points=3000)
    os.makedirs(tmp_path / "model" / "point_cloud" / "iteration_30000")
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: .*--overwrite"):
        run()
    for bad in (["--device", "tpu"], ["--max_steps", "5000"], ["--step", "0"], ["--min_joints", "1"], ["--grid", "6"], ["--grid", "2000"]):
        with pytest.raises(SystemExit, match=r"^trace_strands\.py: "):
            run("--overwrite", *bad)
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: no strand is left"):
        run("--overwrite", "--min_conf", "1e9")
    assert run("--overwrite") > 0
