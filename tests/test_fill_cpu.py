"""The fill of the direction volume without a GPU: the numpy path of utils/field_fill.py against the loop restatement of
tests/fill_reference.py (every tensor entry bit for bit, both returned iterates), an OUT wall, the convex-combination bounds, an
analytic line, classify / seed / quantise / merge, the entry point's refusals and the trace_strands.py --fill driver on a synthetic
capture."""
import ctypes
import os

import numpy as np
import pytest

from tests import fill_cases as FC
from tests import fill_reference as FR
from tests import trace_cases as TC
from tests.test_trace_cpu import DRIVER
from utils import field_fill as FF
from utils import trace as T

_REF = {}


def reference(key, T0, kind, sweeps):
    """{n: the loop's iterate after n sweeps} for n = 0 .. max(sweeps) of a case, computed once and left unchanged."""
    top = max(sweeps)
    if key not in _REF or len(_REF[key]) <= top:
        its = [T0.copy()]
        for _ in range(top):
            its.append(FR.sweep(its[-1], kind))
        for a in its:
            a.setflags(write=False)
        _REF[key] = its
    return _REF[key]


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check_against_loop(fill, key, T0, kind, sweeps):
    its = reference(key, T0, kind, sweeps)
    for n in sweeps:
        res, prev = fill(T0, kind, n)
        assert same_bits(res, its[n]), (key, n)
        assert same_bits(prev, its[max(n - 1, 0)]), (key, n)              # (sweeps = 0: the seed twice)
    return its


@pytest.mark.parametrize("grid", list(FC.GRIDS))
@pytest.mark.parametrize("name", FC.PATTERNS)
def test_numpy_fill_equals_the_restatement(name, grid):
    shape = FC.GRIDS[grid]
    dirs, kind, T0 = FC.pattern(name, shape)
    field = FC.field_of(dirs, kind, shape)
    assert np.array_equal(FF.classify(field, 0.5, kind != FC.OUT), kind)
    assert np.array_equal(FR.classify(field.dir, field.conf, 0.5, kind != FC.OUT), kind)
    seed = FF.seed(field, kind)
    assert same_bits(seed, FR.seed(dirs, kind)) and not seed[:, kind != FC.FIXED].any()
    assert not np.signbit(seed[:, kind != FC.FIXED]).any()                 # +0.0
    its = check_against_loop(FF.fill_numpy, (name, grid), T0, kind, FC.SWEEPS_CPU)
    last = its[max(FC.SWEEPS_CPU)]
    fixed_or_out = kind != FC.FREE
    assert same_bits(last[:, fixed_or_out], T0[:, fixed_or_out])           # FIXED and OUT nodes never change
    if name == "all_free":
        assert not last.any() and not np.signbit(last).any()
    if name == "isolated":
        assert same_bits(last[:, 0, 0, 0], T0[:, 0, 0, 0]) and T0[0, 0, 0, 0] == 0.25      # c = 0: the value is kept
    if name == "minus_zero":
        assert np.signbit(T0).any() and not np.signbit(its[1][:, kind == FC.FREE]).any()   # 0.0 + -0.0 is +0.0
    if name == "negative":
        flipped = FC.field_of(-dirs, kind, shape)
        assert same_bits(FF.seed(flipped, kind), seed)                     # negating a dir changes no bit of the seed
        assert (dirs[kind == FC.FIXED] < 0).any()
    if name == "borders":
        nx, ny, nz = shape
        assert (kind[[0, -1]] == FC.FREE).sum() + (kind[:, [0, -1]] == FC.FREE).sum() + (kind[:, :, [0, -1]] == FC.FREE).sum() >= 8
    if name in ("middle", "thirds", "borders"):
        assert its[1][:, kind == FC.FREE].any()                            # something has diffused


def test_an_out_wall_separates_two_regions():
    dirs, kind = FC.wall()
    shape = FC.GRIDS["g1796"]
    base = FF.fill_numpy(FF.seed(FC.field_of(dirs, kind, shape), kind), kind, 40)[0]
    other_dirs, _ = FC.wall(right=(0.0, 0.6, 0.8))
    other = FF.fill_numpy(FF.seed(FC.field_of(other_dirs, kind, shape), kind), kind, 40)[0]
    assert same_bits(base[:, :, :, :8], other[:, :, :, :8])                # left of the wall: no bit changes
    assert not same_bits(base[:, :, :, 9:], other[:, :, :, 9:])
    assert base[0, :, :, 7].min() > 0.0 and not base[1:, :, :, :8].any()   # left: e_x's tensor alone has arrived, xx and nothing else
    assert base[3, :, :, 9].min() > 0.0 and not base[0, :, :, 9:].any()    # right: e_y's, no xx
    assert not base[:, :, :, 8].any()
    want = FR.fill(FF.seed(FC.field_of(dirs, kind, shape), kind), kind, 3)
    got = FF.fill_numpy(FF.seed(FC.field_of(dirs, kind, shape), kind), kind, 3)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.mark.parametrize("name", ("thirds", "borders", "middle"))
def test_iterates_are_convex_combinations(name):
    shape = FC.GRIDS["g1796"]
    _, kind, T0 = FC.pattern(name, shape)
    for n in (0, 1, 2, 7, 30):
        res = FF.fill_numpy(T0, kind, n)[0]
        trace = (res[0] + res[3]) + res[5]
        assert trace.min() >= 0.0 and trace.max() <= 1.0 + 1e-12
        assert res[0].min() >= 0.0 and res[3].min() >= 0.0 and res[5].min() >= 0.0


def test_analytic_line():
    field, kind = FC.line()
    res, prev = FF.fill_numpy(FF.seed(field, kind), kind, FC.LINE_SWEEPS)
    d, conf = T.solve_numpy(FF.quantise(res))
    FC.check_line(res, d, conf)
    assert np.abs(res - prev).max() <= 1e-12
    merged = FF.merge(field, kind, d, conf)
    assert merged.conf[0, 0, 0] == 1.0 and merged.dir[0, 0, 0].tolist() == [1.0, 0.0, 0.0] and abs(merged.conf[0, 0, 2] - 0.5) <= 1e-9
    stats = {}
    again = FF.fill_field(field, kind, FC.LINE_SWEEPS, stats=stats)
    assert same_bits(again.dir, merged.dir) and same_bits(again.conf, merged.conf) and 0.0 <= stats["last_change"] <= 1e-12


def test_classify_seed_quantise_merge():
    shape = FC.GRIDS["g543"]
    nx, ny, nz = shape
    dirs = FC.unit_dirs(shape, 3)
    conf = np.full((nz, ny, nx), 0.25)
    conf[0, 0, 0], conf[0, 0, 1], conf[0, 0, 2], conf[0, 0, 3] = 0.5, np.nextafter(0.5, 0.0), 0.75, np.nan
    conf[1, 1, 1], conf[1, 1, 2], conf[1, 1, 3] = 2.0, 2.0, 2.0
    dirs[1, 1, 1, 0], dirs[1, 1, 2, 2] = np.nan, np.inf                    # enough mass, but no finite dir: not FIXED
    field = T.Field(TC.ORIGIN, TC.H, shape, dirs, conf)
    kind = FF.classify(field, 0.5)
    assert kind.dtype == np.uint8 and kind.shape == (nz, ny, nx)
    assert kind[0, 0, :4].tolist() == [FC.FIXED, FC.FREE, FC.FIXED, FC.FREE]    # the threshold is met at exactly fixed_conf
    assert kind[1, 1, 1:4].tolist() == [FC.FREE, FC.FREE, FC.FIXED]
    assert FF.counts(kind) == (3, nx * ny * nz - 3, 0)
    allowed = np.zeros((nz, ny, nx), bool)
    allowed[0] = True
    allowed[1, 1, 3] = False
    k2 = FF.classify(field, 0.5, allowed)
    assert np.array_equal(k2, FR.classify(dirs, conf, 0.5, allowed))
    assert k2[1, 1, 3] == FC.FIXED and k2[1, 1, 1] == FC.OUT and k2[0, 0, 1] == FC.FREE and (k2[2] == FC.OUT).all()
    with pytest.raises(ValueError):
        FF.classify(field, 0.5, allowed.astype(np.uint8))
    with pytest.raises(ValueError):
        FF.classify(field, 0.5, allowed[:1])
    # quantise: round-half-even on the 2^-32 grid, the trace summed before the scaling; a T that is not finite is refused by text
    Tq = np.zeros((6, nz, ny, nx))
    Tq[:, 0, 0, 0] = [0.5, 0.25, -0.125, 0.25, 0.0, 0.25]
    Tq[0, 0, 0, 1], Tq[3, 0, 0, 1], Tq[5, 0, 0, 1] = 0.5 * 2.0 ** -32, 1.5 * 2.0 ** -32, 2.5 * 2.0 ** -32
    acc = FF.quantise(Tq)
    assert acc.dtype == np.int64 and acc.shape == (nz, ny, nx, 7)
    assert acc[0, 0, 0].tolist() == [1 << 32, 1 << 31, 1 << 30, -(1 << 29), 1 << 30, 0, 1 << 30]
    assert acc[0, 0, 1].tolist() == [4, 0, 0, 0, 2, 0, 2]                   # halves go to the even neighbour; W = rint(4.5)
    for bad in (np.nan, np.inf, -np.inf):
        Tb = Tq.copy()
        Tb[2, 1, 1, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            FF.quantise(Tb)
    with pytest.raises(ValueError):
        FF.quantise(Tq.astype(np.float32))
    # merge: the FREE nodes take the filled values, every FIXED and OUT node keeps the input's bits -- a NaN conf and a -0.0 included
    field.conf[2, 0, 0], field.dir[2, 0, 0] = np.nan, (-0.0, 0.0, 1.0)
    k2[2, 0, 0] = FC.OUT
    df, cf = FC.unit_dirs(shape, 9), np.full((nz, ny, nx), 0.125)
    merged = FF.merge(field, k2, df, cf)
    free = k2 == FC.FREE
    assert same_bits(merged.dir[free], df[free]) and same_bits(merged.conf[free], cf[free])
    assert same_bits(merged.dir[~free], field.dir[~free]) and same_bits(merged.conf[~free], field.conf[~free])
    assert merged.dir is not field.dir and free.any() and (~free).any()
    for kw in (dict(sweeps=-1), dict(sweeps=65537), dict(sweeps=1.5), dict(kind=k2.astype(np.int32)), dict(kind=k2[:1]), dict(kind=k2 + 2),
               dict(T=Tq.astype(np.float32)), dict(T=Tq[:5])):
        a = dict(T=Tq, kind=k2, sweeps=1)
        a.update(kw)
        with pytest.raises(ValueError):
            FF.fill_numpy(**a)
    assert FF.MAX_SWEEPS == 65536 and (FF.OUT, FF.FREE, FF.FIXED) == (0, 1, 2)


# ---- binding ---------------------------------------------------------------------------------------------------------------
def test_binding_symbol_and_refusals():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    assert hasattr(L, "hgs_field_fill") and len(rt.SIGNATURES["hgs_field_fill"][1]) == 10
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                    # (never dereferenced: every call below is refused first)

    def fill(n=(4, 4, 4), kind=p, index=p, F=4, a=p, b=p + 8, sweeps=3):
        assert L.hgs_field_fill(None, n[0], n[1], n[2], kind, index, F, a, b, sweeps) != 0
        msg = L.hgs_last_error().decode()
        assert msg.startswith("hgs_field_fill: ")
        return msg
    for kw in (dict(kind=None), dict(index=None), dict(a=None), dict(b=None)):
        assert fill(**kw).endswith("are required")
    assert "one buffer" in fill(b=p)
    for n in ((1, 4, 4), (4, 1025, 4), (4, 4, 0), (1024, 1024, 65)):
        assert "a grid of" in fill(n=n)
    assert "free nodes" in fill(F=65) and "free nodes" in fill(F=-1)
    for sweeps in (-1, 65537):
        assert "sweeps" in fill(sweeps=sweeps)
    assert L.hgs_field_fill(None, 4, 4, 4, None, None, 0, None, None, 3) == 0        # F == 0: nothing is launched, no pointer is touched
    assert L.hgs_field_fill(None, 4, 4, 4, None, None, 4, None, None, 0) == 0        # sweeps == 0 likewise
    import torch
    with pytest.raises(rt.HgsError):
        FF.fill_device(torch.zeros(6, 4, 4, 4, dtype=torch.float64), torch.zeros(4, 4, 4, dtype=torch.uint8), 1)   # CPU tensors: no CPU path
    with pytest.raises(rt.HgsError):
        FF.quantise_device(torch.zeros(6, 4, 4, 4, dtype=torch.float64))
    with pytest.raises(rt.HgsError):
        z = torch.zeros(6 * 64, dtype=torch.float64)
        rt.fill_check((4, 4, 4), torch.zeros(64, dtype=torch.uint8), z, z.clone(), torch.zeros(4, dtype=torch.int32))


# ---- the driver --------------------------------------------------------------------------------------------------------------
BOX = ["--fill", str(FC.FILL), "--fill_domain", "box"]


def last_joint_radii(model, n, points=12):
    from utils.ply import read_ply
    v = dict(read_ply(str(model / "point_cloud" / "iteration_1" / "point_cloud.ply")))["vertex"]
    J = np.stack([np.asarray(v[c], np.float64) for c in "xyz"], axis=1).reshape(n, points, 3)
    return np.linalg.norm(J[:, -1], axis=1)


def kind_counts(out):
    import re
    m = re.search(r"fill \((hull|box)\): (\d+) fixed, (\d+) free, (\d+) out node\(s\)", out)
    return tuple(int(m.group(k)) for k in (2, 3, 4))


def test_driver_fills_the_gap(tmp_path, capsys):
    """tests/fill_cases.py states how the gap and the sweeps were chosen; the two conditions below are conditions on that scene."""
    import trace_strands as driver
    src = tmp_path / "scene"
    FC.write_scene(src)
    run = lambda m, *extra: driver.main(["-s", str(src), "-m", str(tmp_path / m)] + DRIVER + list(extra))      # noqa: E731
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: no strand is left"):
        run("plain")                                             # the gap exceeds --max_gap steps: every root dies in it
    capsys.readouterr()
    n = run("filled", "--field", str(tmp_path / "field.npz"), *BOX)
    out = capsys.readouterr().out
    radii = last_joint_radii(tmp_path / "filled", n)
    assert n >= 0.9 * FC.ROOTS and int((radii > 0.7).sum()) >= 0.9 * FC.ROOTS, (n, np.sort(radii)[:10])
    # the printed counts are those of the saved volume's grid, and the recomputed kinds' own
    field = T.load_field(str(tmp_path / "field.npz"))
    fixed, free, out_nodes = kind_counts(out)
    nodes = field.shape[0] * field.shape[1] * field.shape[2]
    assert fixed + free + out_nodes == nodes and fixed > 500 and free > 5000 and out_nodes > 100
    from utils import head_sdf as H
    sdf = H.load_sdf(H.scene_sdf_path(str(src)))
    allowed = driver.fill_allowed(str(src), field, sdf, 0.0, "box", 3, 50, None)
    inside = ~allowed
    assert out_nodes <= int(inside.sum()) and (field.conf[inside] == 0).all()      # (a node inside the head is OUT, or was FIXED and cleared: none is)
    assert out_nodes == int(inside.sum())
    assert "scalp point(s) splatted" in out and f"{FC.FILL} sweep(s): the last one changed an entry by" in out
    assert f"of {free} free node(s) ended with at least 0.5" in out
    assert ((field.conf >= 0.0) & np.isfinite(field.conf)).all()
    # without the scalp's nodes the fixed count drops by the nodes taken from them
    capsys.readouterr()
    run("no_scalp", "--no_fill_scalp", "--min_joints", "2", *BOX)
    out2 = capsys.readouterr().out
    assert "scalp point(s) splatted" not in out2 and kind_counts(out2)[0] < fixed


def test_fill_zero_is_the_plain_driver(tmp_path):
    import trace_strands as driver
    src = tmp_path / "scene"
    FC.write_scene(src, shell=(0.5, 0.85))                       # no gap: strands survive without the fill
    ply = lambda m: tmp_path / m / "point_cloud" / "iteration_1" / "point_cloud.ply"       # noqa: E731
    n = driver.main(["-s", str(src), "-m", str(tmp_path / "plain")] + DRIVER)
    assert driver.main(["-s", str(src), "-m", str(tmp_path / "zero"), "--fill", "0", "--fill_domain", "box", "--no_fill_scalp"] + DRIVER) == n
    with open(ply("plain"), "rb") as a, open(ply("zero"), "rb") as b:
        assert n > 30 and a.read() == b.read()


def test_driver_refusals(tmp_path):
    import shutil
    import trace_strands as driver
    src = tmp_path / "scene"
    FC.write_scene(src, sdf=False)
    run = lambda *extra: driver.main(["-s", str(src), "-m", str(tmp_path / "model")] + DRIVER + list(extra))     # noqa: E731
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: .*head_sdf\.npz is missing.*head_sdf\.py"):
        run(*BOX)
    FC.write_scene(src)
    shutil.rmtree(src / "masks")
    with pytest.raises(SystemExit, match=r"^trace_strands\.py: .*masks/.*--fill_domain box"):
        run("--fill", "5")
    for bad in (["--fill", "-1"], ["--fill", "65537"], ["--fill", "5", "--fill_min_views", "0"], ["--fill", "5", "--fill_min_percent", "101"],
                ["--fill", "5", "--fill_fixed_conf", "nan"]):
        with pytest.raises(SystemExit, match=r"^trace_strands\.py: "):
            run(*bad)
    assert not os.path.exists(tmp_path / "model")                # (refused before anything is written)


def test_hull_domain_votes_on_the_masks(tmp_path, capsys):
    import trace_strands as driver
    from data import capture
    from utils import carve
    from utils import head_sdf as H
    from utils.views import load_views, read_plane
    from tests import head_sdf_cases as HC
    src = tmp_path / "scene"
    TC.write_scene(src)                                          # two 64 x 64 views with masks
    v, f = HC.uv_sphere(rings=12, segments=16, radius=0.5, centre=(0.0, 0.0, 0.0))
    sdf = H.build_sdf(v, f, grid=24, pad=0.1)
    H.save_sdf(H.scene_sdf_path(str(src)), sdf)
    rule = ["--fill_min_views", "1", "--fill_min_percent", "50"]
    n = driver.main(["-s", str(src), "-m", str(tmp_path / "model"), "--field", str(tmp_path / "field.npz"), "--fill", "10"] + rule + DRIVER)
    out = capsys.readouterr().out
    field = T.load_field(str(tmp_path / "field.npz"))
    allowed = driver.fill_allowed(str(src), field, sdf, 0.0, "hull", 1, 50, None)
    views = load_views(str(src / "sparse" / "0"))
    masks = [read_plane(capture.mask_path(str(src), capture.file_name(view)), view, "the mask") for view in views]
    seen, hits = carve.mask_votes(field.nodes(), views, masks)
    voted = carve.keep(seen, hits, 1, 50).reshape(allowed.shape)
    outside = H.sample(field.nodes().astype(np.float32), sdf, 0.0)[2].reshape(allowed.shape) >= 0
    assert np.array_equal(allowed, voted & outside) and 0 < voted.sum() < voted.size and (voted & ~outside).any()
    fixed, free, out_nodes = kind_counts(out)
    assert "fill (hull)" in out and n > 0 and fixed + free + out_nodes == allowed.size
    assert free <= int(allowed.sum()) and out_nodes >= int((~allowed).sum()) - fixed and out_nodes > 0
    strict = driver.fill_allowed(str(src), field, sdf, 0.0, "hull", 3, 50, None)
    assert not strict.any()                                      # two views cannot meet the default of three
