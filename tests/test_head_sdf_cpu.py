"""The head's distance field and the penetration term without a GPU: the numpy paths of utils/head_sdf.py against the float64
restatement of tests/head_sdf_reference.py (|phi| bit for bit, signs by decision, the float32 term under the K = 8 comparator), the
torch statement of loss/losses.py against the numpy path, the file, the entry points' refusals, the options and the drivers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import head_sdf_cases as HC
from tests import head_sdf_reference as HR
from utils import head_sdf as H

_BUILT = {}


def built(name):
    """(sdf, stats, reference magnitude, reference winding, dropped, degenerate) of a mesh case, computed once."""
    if name not in _BUILT:
        verts, faces, grid, pad = HC.mesh_cases()[name]
        stats = {"winding": None}
        sdf = H.build_sdf(verts, faces, grid=grid, pad=pad, stats=stats)
        mag, w, dropped, degenerate = HR.field(verts, faces, sdf.origin, sdf.spacing, sdf.shape)
        _BUILT[name] = (sdf, stats, mag, w, dropped, degenerate)
    return _BUILT[name]


@pytest.mark.parametrize("name", HC.MESH_NAMES)
def test_numpy_field_against_the_restatement(name):
    sdf, stats, mag, w, dropped, degenerate = built(name)
    assert np.abs(sdf.phi).tobytes() == mag.astype(np.float32).tobytes()                 # |phi|: equal bits
    assert (stats["dropped"], stats["degenerate"]) == (dropped, degenerate)
    sure = HR.decided(w, HC.NEAR)
    assert ((sdf.phi < 0) == (w > 0.5))[sure].all()
    assert not np.signbit(sdf.phi[sdf.phi == 0]).any()                                    # a zero is +0
    assert np.abs(stats["winding"] - w).max() < 1e-12


@pytest.mark.parametrize("name", HC.MESH_NAMES)
def test_the_cases_decide_their_signs(name):
    """The nodes within 1e-9 of w = 0.5 are at most 0.1 % of a case's nodes, none for the closed meshes (w is an integer off the
    surface); a closed mesh has nodes inside, and w = 1 there."""
    _, _, _, w, _, _ = built(name)
    near = int((~HR.decided(w, HC.NEAR)).sum())
    assert near <= HC.NEAR_SHARE * w.size, (near, w.size)
    if name in HC.CLOSED:
        assert near == 0
        assert np.abs(w - np.round(w)).max() < 1e-9
    if not name.endswith("_g2"):                     # (a grid of 2 has the box's corners only: all outside)
        assert w.max() > 0.999 or name not in HC.CLOSED
        assert (w > 0.5).any() and (w < 0.5).any()


def test_grid_shapes_and_box():
    sdf = built("flat_cube_g17")[0]
    nx, ny, nz = sdf.shape
    assert nx == 17 and ny < nx and nz < ny and sdf.phi.shape == (nz, ny, nx)             # clearly not cubic
    assert built("tetra_g2")[0].shape[0] >= 2 and np.prod(built("tetra_g5")[0].shape) % 64 != 0
    sdf = built("dirty_cube_g5")[0]
    assert built("dirty_cube_g5")[1]["faces"] == 13 and (sdf.mesh_faces, sdf.mesh_verts) == (15, 9)
    np.testing.assert_allclose(sdf.origin, [-1.2, -1.2, -1.2])
    assert abs(sdf.spacing - 0.6) < 1e-12 and sdf.shape == (5, 5, 5)
    # the duplicated face changes the winding number, the distance does not mind it
    assert np.abs(sdf.phi).tobytes() == np.abs(built("cube_g5")[0].phi).tobytes()
    v, f = HC.cube()
    for bad in (dict(grid=1), dict(grid=513), dict(pad=-0.1), dict(pad=float("nan"))):
        with pytest.raises(ValueError):
            H.build_sdf(v, f, **{"grid": 5, "pad": 0.1, **bad})
    with pytest.raises(ValueError, match="no usable face"):
        H.build_sdf(np.concatenate([v, [[np.nan] * 3]]), np.array([[0, 1, 8], [0, 3, 3]]), grid=5)
    with pytest.raises(ValueError):
        H.build_sdf(v, np.array([[0, 1, 9]]), grid=5)                                     # (utils.scalp.check_mesh)


def test_sphere_field_is_a_distance():
    """Against the analytic sphere: the faceted mesh lies inside it by at most r (1 - cos(pi / 16)) plus the chord sag."""
    sdf = built("sphere_g17")[0]
    nx, ny, nz = sdf.shape
    z, y, x = np.meshgrid(*(sdf.origin[k] + sdf.spacing * np.arange(n) for k, n in ((2, nz), (1, ny), (0, nx))), indexing="ij")
    exact = np.sqrt((x - 0.03) ** 2 + (y + 0.02) ** 2 + (z - 0.05) ** 2) - 0.8
    assert np.abs(sdf.phi - exact).max() < 0.8 * (1 - np.cos(np.pi / 16)) * 2.5


# ---- the term ----------------------------------------------------------------------------------------------------------
_POINTS = {}


def point_case(name):
    if name not in _POINTS:
        field, pts, margin = HC.point_cases()[name]
        _POINTS[name] = (HC.FIELDS[field](), pts, margin)
    return _POINTS[name]


@pytest.mark.parametrize("name", HC.POINT_NAMES)
def test_numpy_term_against_float64(name):
    sdf, pts, margin = point_case(name)
    pen, g, d, ok = H.sample(pts, sdf, margin)
    p64, g64, d64, ok64 = HR.sample(pts, sdf, margin)
    assert pen.dtype == np.float32 and g.dtype == np.float32 and g.shape == pts.shape
    assert (ok == ok64).all() and np.isinf(d[~ok]).all() and (pen[~ok] == 0).all() and (g[~ok] == 0).all()
    # per point, within what the statement's own roundings allow (HR.error_bounds): r is off by e_d, so pen = r r by 2 |r| e_d + e_d^2
    # and g = -2 r grad by 2 e_d |grad| + 2 |r| e_grad, each with a few roundings of its own on top
    e_d, e_grad = HR.error_bounds(sdf)
    u = 2.0 ** -24
    r64 = np.where(ok, np.float64(np.float32(margin)) - np.where(ok, d64, 0.0), 0.0)
    assert (np.abs(d[ok] - d64[ok]) <= e_d).all()
    assert (np.abs(pen - p64) <= 2 * np.abs(r64) * e_d + e_d ** 2 + 4 * u * p64).all()
    k = float(sdf.inv_h32)
    D = max(float(np.abs(np.diff(sdf.phi.astype(np.float64), axis=a)).max()) for a in range(3))
    assert (np.abs(g - g64) <= (2 * e_d * D * k + 2 * np.abs(r64) * e_grad + 4 * u * np.abs(g64).max(initial=0.0))[:, None]).all()
    for upstream in (1.0, 0.37):
        L, grad = H.penalty(pts, sdf, margin, upstream)
        assert L.dtype == np.float32 and grad.dtype == np.float32
        E = pts.shape[0]
        if E:
            assert L == np.float32(pen.astype(np.float64).sum() / E)
            assert grad.tobytes() == (g * (np.float32(upstream) / np.float32(E))).tobytes()      # one division, one multiplication
        # the comparator: the numpy path is its own yardstick here, the ratios are 1 at most; the device op is held to K = 8
        rv, rg = HR.ratios(L, grad, pts, sdf, margin, upstream)
        assert rv <= 1.0 and rg <= 1.0 and HR.accepts(L, grad, pts, sdf, margin, upstream)


def test_special_points_are_what_they_claim():
    sdf, pts, _ = point_case("ball_special")
    pen, g, d, ok = H.sample(pts, sdf, 0.0)
    t = (pts - sdf.origin32) * sdf.inv_h32
    assert (t[:4] == np.round(t[:4])).all() and ok[:4].all()                              # nodes, exactly
    assert d[:4].tobytes() == np.array([sdf.phi[4, 6, 8], sdf.phi[4, 5, 9], sdf.phi[0, 0, 0], sdf.phi[7, 11, 15]]).tobytes()
    assert ((t[4:7] == np.round(t[4:7])).sum(axis=1) >= 1).all() and ok[4:7].all()        # cell faces
    assert (t[7] == [16, 12, 8]).all() and not ok[7:11].any()                             # t = n - 1 exactly: out of range
    assert ok[11] and not ok[12:20].any()
    assert (d[20:23] < 0).all() and (d[20:23] > -0.125).all() and (d[23:26] < -0.125).all() and (pen[20:26] > 0).all()
    assert (d[26:28] > 0).all() and (pen[26:28] == 0).all()
    pen_m = H.sample(pts, sdf, 0.05)[0]
    assert (pen_m[26:28] > 0).all()                                                       # within the margin
    L, grad = H.penalty(point_case("ball_all_outside")[1], sdf, 0.05)
    assert L == 0 and not grad.any() and not np.signbit(L)
    assert H.penalty(np.zeros((0, 3), np.float32), sdf, 0.0)[0] == 0


def test_gradient_against_central_differences():
    """Inside a cell, away from r = 0, the analytic gradient is the derivative of pen: central differences of the float64 restatement
    (step 1e-4 of a cell of 0.125: the interpolant is a cubic polynomial there, the truncation error ~ step^2)."""
    sdf, pts, _ = point_case("ball_special")
    for margin in (0.0, 0.05):
        _, g64, d64, ok = HR.sample(pts, sdf, margin)
        checked = 0
        for e in np.nonzero(ok)[0]:
            t = (pts[e].astype(np.float64) - sdf.origin32) * np.float64(sdf.inv_h32)
            frac = t - np.floor(t)
            if frac.min() < 0.01 or frac.max() > 0.99 or abs(margin - d64[e]) < 0.01 or d64[e] > margin:
                continue
            fd = HR.central_difference(pts[e], sdf, margin, 1e-5)
            assert np.abs(fd - g64[e]).max() <= 1e-6 * max(1.0, np.abs(g64[e]).max()), (e, fd, g64[e])
            checked += 1
        assert checked >= 4


class _Model:
    def __init__(self, pts):
        self._endpoints = torch.tensor(pts, dtype=torch.float32, requires_grad=True)


@pytest.mark.parametrize("name", HC.POINT_NAMES)
def test_torch_statement_against_the_numpy_path(name):
    from loss.losses import head_penetration_loss
    sdf, pts, margin = point_case(name)
    m = _Model(pts)
    L = head_penetration_loss(m, sdf, margin)
    (L * 0.37).backward()
    Ln, gn = H.penalty(pts, sdf, margin, 0.37)
    E = pts.shape[0]
    grad = m._endpoints.grad.numpy() if E else np.zeros((0, 3), np.float32)
    # the value: float32 pen, bit-equal per point, summed in float32 here and in float64 there: E ulp of the sum at the very most
    assert abs(float(L.detach()) - float(Ln)) <= max(E, 1) * 2.0 ** -23 * float(Ln)
    assert np.isfinite(grad).all()
    rv, rg = HR.ratios(np.float32(Ln), grad, pts, sdf, margin, 0.37)
    print(f"ratio | head torch statement | {name} | gradient {rg:.2f} |")
    assert rg <= HR.K, rg


# ---- the file ------------------------------------------------------------------------------------------------------------
def test_npz_round_trip_and_refusals(tmp_path):
    sdf = built("flat_cube_g17")[0]
    path = str(tmp_path / "head_sdf.npz")
    H.save_sdf(path, sdf)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(H.KEYS)
    back = H.load_sdf(path)
    assert back.shape == sdf.shape and back.spacing == sdf.spacing and back.origin.tobytes() == sdf.origin.tobytes()
    assert back.phi.tobytes() == sdf.phi.tobytes() and (back.mesh_faces, back.mesh_verts) == (12, 8)
    good = dict(origin=sdf.origin, spacing=np.float64(sdf.spacing), shape=np.asarray(sdf.shape), phi=sdf.phi, mesh_faces=np.int64(12),
                mesh_verts=np.int64(8))
    bad = str(tmp_path / "bad.npz")
    for change in (dict(extra=np.zeros(1)), dict(phi=None), dict(phi=sdf.phi.astype(np.float64)), dict(phi=sdf.phi[:-1]),
                   dict(shape=np.asarray(sdf.shape[::-1])), dict(spacing=np.float64(0.0)), dict(origin=np.array([0.0, np.nan, 0.0])),
                   dict(origin=np.zeros(4)), dict(mesh_faces=np.float64(1.5))):
        np.savez(bad, **{k: v for k, v in {**good, **change}.items() if v is not None})
        with pytest.raises(ValueError, match="bad.npz"):
            H.load_sdf(bad)
    with open(bad, "wb") as fh:
        fh.write(b"not an archive")
    with pytest.raises(ValueError, match="not a head distance field"):
        H.load_sdf(bad)


# ---- binding, options, drivers -------------------------------------------------------------------------------------------
def test_binding_symbols_and_refusals():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    want = {"hgs_mesh_sdf": 12, "hgs_head_penalty_num_blocks": 1, "hgs_head_penalty_forward": 17, "hgs_head_penalty_backward": 5}
    for name, n_args in want.items():
        assert hasattr(L, name) and len(rt.SIGNATURES[name][1]) == n_args
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                                             # (never dereferenced: every call below is refused first)

    def sdf(F=1, tris=p, o=(0.0, 0.0, 0.0), h=0.1, n=(4, 4, 4), phi=p, w=None):
        assert L.hgs_mesh_sdf(None, F, tris, o[0], o[1], o[2], h, n[0], n[1], n[2], phi, w) != 0
        return L.hgs_last_error().decode()

    def fwd(E=4, pts=p, phi=p, n=(4, 4, 4), o=(0.0, 0.0, 0.0), k=10.0, margin=0.0, g=p, pen=None, dist=None, partials=p, out=p):
        assert L.hgs_head_penalty_forward(None, E, pts, phi, n[0], n[1], n[2], o[0], o[1], o[2], k, margin, g, pen, dist, partials, out) != 0
        return L.hgs_last_error().decode()

    def bwd(E=4, g=p, up=p, d=p):
        assert L.hgs_head_penalty_backward(None, E, g, up, d) != 0
        return L.hgs_last_error().decode()
    for F in (0, -1, (1 << 24) + 1):
        assert sdf(F=F).startswith("hgs_mesh_sdf: ") and "faces" in sdf(F=F)
    for n in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert "a grid of" in sdf(n=n) and "a grid of" in fwd(n=n)
    for h in (0.0, -1.0, float("inf"), float("nan")):
        assert "spacing" in sdf(h=h)
    assert "origin" in sdf(o=(float("nan"), 0.0, 0.0))
    assert sdf(tris=None).endswith("are required") and sdf(phi=None).endswith("are required")
    assert "points" in fwd(E=-1) and "points" in fwd(E=(1 << 28) + 1)
    for k in (0.0, -1.0, float("inf"), float("nan")):
        assert "1/h" in fwd(k=k)
    assert "margin" in fwd(margin=float("nan")) and "origin" in fwd(o=(0.0, float("inf"), 0.0))
    for kw in (dict(pts=None), dict(g=None), dict(partials=None), dict(phi=None), dict(out=None)):
        assert fwd(**kw).endswith("are required")
    assert "points" in bwd(E=-1)
    for kw in (dict(g=None), dict(up=None), dict(d=None)):
        assert bwd(**kw).endswith("are required")
    assert L.hgs_head_penalty_backward(None, 0, None, None, None) == 0                    # E == 0 launches nothing
    assert [L.hgs_head_penalty_num_blocks(E) for E in (-1, 0, 1, 256, 257)] == [0, 0, 1, 1, 2]
    from hgs_runtime.fused import head_penalty
    with pytest.raises(rt.HgsError):
        head_penalty(torch.zeros(4, 3), HC.ball_field(), 0.0)                             # CPU tensors: there is no CPU path


def test_options_default_to_off():
    from argparse import ArgumentParser
    from arguments import OptimizationParams
    op = OptimizationParams()
    assert op.lambda_head == 0 and op.head_margin == 0
    parser = ArgumentParser()
    got = OptimizationParams(parser).extract(parser.parse_args(["--lambda_head", "0.5", "--head_margin", "0.002"]))
    assert got.lambda_head == 0.5 and got.head_margin == 0.002


def test_train_without_the_field_names_the_tool(tmp_path):
    import train as train_cli
    with pytest.raises(SystemExit, match=r"head_sdf\.npz.*head_sdf\.py"):
        train_cli.main(["-s", str(tmp_path), "-m", str(tmp_path / "out"), "--lambda_head", "1"])
    assert not os.path.exists(tmp_path / "out")                                           # (refused before anything is written)
    with open(tmp_path / "head_sdf.npz", "wb") as fh:
        fh.write(b"junk")
    with pytest.raises(SystemExit, match="not a head distance field"):
        train_cli.main(["-s", str(tmp_path), "-m", str(tmp_path / "out"), "--lambda_head", "1"])


def _strand_ply(path, strands):
    from scene.hair_gaussian_model import HairGaussianModel
    m = HairGaussianModel.from_strands(np.asarray(strands, np.float32), sh_degree=0, device="cpu", ref_strand_root=np.asarray(strands, np.float32)[:, 0])
    m.save_ply(str(path))
    return m


def test_driver_on_cpu_and_report(tmp_path, capsys):
    import head_sdf as driver
    from tests.scalp_cases import write_ply
    src = tmp_path / "scene"
    os.makedirs(src)
    with pytest.raises(SystemExit, match=r"^head_sdf\.py: .*head_mesh\.ply is missing"):
        driver.main(["-s", str(src), "--device", "cpu"])
    verts, faces = HC.uv_sphere()
    write_ply(str(src / "head_mesh.ply"), verts, faces)
    sdf = driver.main(["-s", str(src), "--device", "cpu", "--grid", "9"])
    out = capsys.readouterr().out
    assert "480 faces: 480 used, 0 dropped" in out and "0 degenerate" in out and " h " in out and "box" in out
    back = H.load_sdf(str(src / "head_sdf.npz"))
    assert back.phi.tobytes() == sdf.phi.tobytes() and back.shape == sdf.shape and (back.phi < 0).any()
    assert [f for f in os.listdir(src) if ".tmp" in f] == []
    with pytest.raises(SystemExit, match=r"^head_sdf\.py: .*--overwrite"):
        driver.main(["-s", str(src), "--device", "cpu", "--grid", "9"])
    driver.main(["-s", str(src), "--device", "cpu", "--grid", "9", "--overwrite"])
    with pytest.raises(SystemExit, match=r"^head_sdf\.py: "):
        driver.main(["-s", str(src), "--device", "cpu", "--grid", "1", "--overwrite"])
    with pytest.raises(SystemExit, match=r"^head_sdf\.py: "):
        driver.main(["-s", str(src), "--device", "tpu"])
    # a hand-placed strand: 5 joints, from the sphere's centre straight out along x in steps of 0.3: three inside (0, 0.3, 0.6 < 0.8)
    c = np.array([0.03, -0.02, 0.05])
    strand = c[None, :] + np.array([[0.3 * k, 0.0, 0.0] for k in range(5)])
    outside = c[None, :] + np.array([[0.0, 1.0 + 0.05 * k, 0.0] for k in range(5)])
    ply = tmp_path / "model" / "point_cloud" / "iteration_3" / "point_cloud.ply"
    os.makedirs(ply.parent)
    _strand_ply(ply, [strand, outside])
    for target in (str(tmp_path / "model"), str(ply)):
        st = driver.main(["-s", str(src), "--device", "cpu", "--report", target])
        assert st["joints"] == 10 and st["inside"] == 3 and abs(st["share"] - 0.3) < 1e-12
        assert 0.6 < st["deepest"] < 0.8 + 1e-6 and 0 < st["mean_depth"] < st["deepest"]
    assert "3 inside the head (30.000 %)" in capsys.readouterr().out
    with pytest.raises(SystemExit, match=r"^head_sdf\.py: "):
        driver.main(["-s", str(src), "--device", "cpu", "--report", str(src / "head_mesh.ply")])


def test_term_is_absent_when_off_and_present_when_on():
    """loss_function adds terms["head"] only with lambda_head > 0, on a strand model that carries a field (the CPU route of the op-by-op
    path: loss_function takes a rendered image, so no rasterizer is needed); a model that is no strand model gets no term."""
    from types import SimpleNamespace
    from arguments import OptimizationParams
    from loss import losses as Ls
    from scene.hair_gaussian_model import HairGaussianModel
    c = HC.CENTRE
    strands = np.stack([c[None, :] + np.array([[0.1 * k, 0.02 * s, 0.0] for k in range(6)]) for s in range(3)]).astype(np.float32)
    m = HairGaussianModel.from_strands(strands, sh_degree=0, device="cpu", ref_strand_root=strands[:, 0])
    img = torch.rand(3, 8, 8)
    cam = SimpleNamespace(original_image=torch.rand(3, 8, 8), mask=None)
    opt = OptimizationParams()
    opt.lambda_orientation = 0.0
    opt.lambda_smooth = 0.0
    _, terms = Ls.loss_function(m, img, cam, opt)
    assert "head" not in terms
    m.head_sdf = HC.ball_field()
    _, terms = Ls.loss_function(m, img, cam, opt)
    assert "head" not in terms                                                            # lambda_head = 0: no term, whatever the model carries
    opt.lambda_head, opt.head_margin = 2.0, 0.01
    loss, terms = Ls.loss_function(m, img, cam, opt)
    want, _ = H.penalty(strands.reshape(-1, 3), m.head_sdf, 0.01)
    head = float(terms["head"].detach())
    assert head > 0 and abs(head - float(want)) <= 18 * 2.0 ** -23 * float(want)
    base = max(0, 1.0 - opt.lambda_dssim) * terms["l1"] + opt.lambda_dssim * terms["dssim"]
    assert abs(float(loss.detach()) - float((base + 2.0 * terms["head"]).detach())) <= 1e-6 * float(loss.detach())
    _, terms = Ls.loss_function(SimpleNamespace(head_sdf=m.head_sdf), img, cam, opt)      # a Stage-I cloud: no term, as with smoothness
    assert "head" not in terms
    # (loss_function_single_pass needs the rasterizer: tests/test_head_sdf_gpu.py::test_switch_and_step_surface has its two sides)
