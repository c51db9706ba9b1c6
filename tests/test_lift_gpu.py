"""hgs_lift_moments and hgs_lift_solve (csrc/hgs_lift.hip) against the numpy path of utils/lift.py: the moments bit for bit, at point
counts around the 64-lane wavefront and the 256-lane workgroup, with 1 / 2 / 8 views of two sizes, with and without a previous
direction, the degenerate points included; the Jacobi solve against numpy.linalg.eigh under the rule of lift_cases.compare_solves;
repeatability; the refusals; the init_cloud.py --directions driver on both devices; and a model initialised from the directions."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import carve_cases as CC
from tests import lift_cases as LC

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 1000)
VS = (1, 2, 8)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cases():
    """{V: (views, planes, Packed, points, prev, host moments without prev, host moments with prev)} at the largest N, computed once;
    a smaller N is a prefix of it (a point's sums do not depend on the other points)."""
    from utils import lift
    out = {}
    s2 = lift.sin2(10.0)
    for V in VS:
        views = LC.equality_views(V)
        planes = LC.random_planes(views, seed=V)
        pts, prev = LC.equality_points(max(NS)), LC.unit_prev(max(NS))
        out[V] = (views, planes, lift.pack(views, *planes, "cuda"), pts, prev, lift.moments_numpy(pts, views, *planes),
                  lift.moments_numpy(pts, views, *planes, prev, s2))
    return out


# ---- 1. moments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_moments_equal_the_numpy_path(cases, N):
    from utils import lift
    s2 = lift.sin2(10.0)
    for V in VS:
        views, planes, packed, pts, prev, plain, robust = cases[V]
        dev = torch.from_numpy(pts[:N]).cuda()
        got = lift.moments_device(dev, packed)
        assert got[0].shape == (N, 6) and got[0].dtype == got[1].dtype == torch.float64 and got[2].dtype == torch.int32
        assert all(_bits(g.cpu().numpy(), w[:N]) for g, w in zip(got, plain)), (V, "no prev")
        got = lift.moments_device(dev, packed, torch.from_numpy(prev[:N]).cuda(), s2)
        assert all(_bits(g.cpu().numpy(), w[:N]) for g, w in zip(got, robust)), (V, "prev")
        if N == max(NS):
            assert plain[2].sum() > 0 and (plain[2] < V).any() and not _bits(plain[0], robust[0])
            for min_conf in (0, 100):
                want = lift.moments_numpy(pts, views, *planes, prev, s2, min_conf)
                got = lift.moments_device(dev, packed, torch.from_numpy(prev).cuda(), s2, min_conf)
                assert all(_bits(g.cpu().numpy(), w) for g, w in zip(got, want)), (V, min_conf)
    if N:                                                        # the host-array entry point
        views, planes, packed, pts, prev, plain, robust = cases[2]
        host = lift.lift_moments(pts[:N], views, *planes, prev[:N], s2, device="cuda")
        assert all(_bits(a, b[:N]) for a, b in zip(host, robust))


def test_border_points_through_the_identity_view():
    from utils import lift
    W, H = CC.SIZES[0]
    v = [CC.identity_view(W, H)] * 2
    full = np.full((H, W), 255, np.uint8)
    orients = [np.full((H, W), 40, np.uint8), np.full((H, W), 90, np.uint8)]
    pts, seen = CC.border_points(W, H)
    d, coh, count = lift.lift_directions(pts, v, [full] * 2, orients, [full] * 2, device="cuda")
    assert np.array_equal(count, 2 * seen) and np.isfinite(d).all() and np.isfinite(coh).all() and not d[seen == 0].any()
    assert np.allclose(np.linalg.norm(d[seen == 1], axis=1), 1.0, rtol=0, atol=1e-12)
    want = lift.lift_moments(pts, v, [full] * 2, orients, [full] * 2)
    assert all(_bits(a, b) for a, b in zip(lift.lift_moments(pts, v, [full] * 2, orients, [full] * 2, device="cuda"), want))


# ---- 2. solve ----------------------------------------------------------------------------------------------------------------------
def test_solve_agrees_with_eigh(cases):
    from utils import lift
    below = rows = 0
    for V in VS:
        for M, _, count in cases[V][5:7]:
            host = lift.solve_numpy(M, count)
            live = host[0].any(axis=1)
            assert (LC.relative_gap(M)[live] >= 1e-6).all()      # the generic inputs have no row below the gap on the host path alone
            dev = tuple(t.cpu().numpy() for t in lift.solve_device(torch.from_numpy(M).cuda(), torch.from_numpy(count).cuda()))
            below += LC.compare_solves(M, dev, host)
            rows += int(live.sum())
            for min_views in (3, 9):                             # the flag follows count
                h = lift.solve_numpy(M, count, min_views)
                g = tuple(t.cpu().numpy() for t in lift.solve_device(torch.from_numpy(M).cuda(), torch.from_numpy(count).cuda(), min_views))
                assert np.array_equal(g[0].any(axis=1), h[0].any(axis=1)) and not g[0][count < min_views].any()
                assert not g[1][count < min_views].any()
    print(f"{below} of {rows} rows below the gap")
    assert rows > 500 and below <= 0.01 * rows
    # rank-deficient and non-finite matrices: unit or zero length, finite
    e = np.array([0.6, 0.0, 0.8])
    outer = np.outer(e, e)
    rank1 = [outer[0, 0], outer[0, 1], outer[0, 2], outer[1, 1], outer[1, 2], outer[2, 2]]
    hard = np.array([[0.0] * 6, rank1, [1.0, 0, 0, 1.0, 0, 1.0], [1.0, 0, 0, 1.0, 0, 2.0], [np.inf, 0, 0, 1.0, 0, 1.0], [1.0, np.nan, 0, 1.0, 0, 1.0],
                     [1e-300, 0, 0, 2e-300, 0, 3e-300], [1e300, 0, 0, 2e300, 0, 3e300]])
    cnt = np.full(len(hard), 4, np.int32)
    d, coh = (t.cpu().numpy() for t in lift.solve_device(torch.from_numpy(hard).cuda(), torch.from_numpy(cnt).cuda()))
    assert np.isfinite(d).all() and np.isfinite(coh).all()
    norm = np.linalg.norm(d, axis=1)
    assert ((norm == 0) | (np.abs(norm - 1.0) < 1e-12)).all()
    assert norm[0] == 0 and norm[4] == 0 and norm[5] == 0 and norm[2] == 1 and norm[6] == 1 and norm[7] == 1
    assert d[6].tolist() == [1.0, 0.0, 0.0] and abs(coh[6] - 1.0 / 3.0) < 1e-15 and abs(coh[7] - 1.0 / 3.0) < 1e-15
    hd, hc = lift.solve_numpy(hard, cnt)
    assert np.array_equal(norm[[0, 2, 3, 4, 5, 6, 7]] == 0, np.linalg.norm(hd, axis=1)[[0, 2, 3, 4, 5, 6, 7]] == 0)


# ---- 3. repeatability ----------------------------------------------------------------------------------------------------------
def test_repeatable_and_stream_independent(cases):
    from utils import lift
    views, planes, packed, pts, prev, _, _ = cases[8]
    dev, p = torch.from_numpy(pts).cuda(), torch.from_numpy(prev).cuda()

    def run():
        M, wsum, count = lift.moments_device(dev, packed, p, lift.sin2(10.0))
        return (M, wsum, count) + lift.solve_device(M, count) + lift.directions_device(dev, packed, 2)
    a, b = run(), run()
    assert all(_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    assert all(_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, c))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(cases):
    import hgs_runtime as rt
    from utils import carve, lift
    views, planes, packed, pts, prev, _, _ = cases[2]
    dev = torch.from_numpy(pts[:8]).cuda()
    p = torch.from_numpy(prev[:8]).cuda()
    L, st = rt.lib(), rt.current_stream()
    M = torch.zeros((8, 6), dtype=torch.float64, device="cuda")
    wsum = torch.zeros(8, dtype=torch.float64, device="cuda")
    count = torch.zeros(8, dtype=torch.int32, device="cuda")
    d = torch.zeros((8, 3), dtype=torch.float64, device="cuda")
    coh = torch.zeros(8, dtype=torch.float64, device="cuda")
    good = dict(N=8, points=rt.ptr(dev), V=2, views=rt.ptr(packed.carve.views_dev), masks=rt.ptr(packed.carve.masks_dev),
                orients=rt.ptr(packed.orients_dev), confs=rt.ptr(packed.confs_dev), tab=rt.ptr(packed.tab_dev), prev=rt.ptr(p),
                s2=0.03, min_conf=1, M=rt.ptr(M), wsum=rt.ptr(wsum), count=rt.ptr(count))

    def moments(**change):
        a = dict(good, **change)
        return L.hgs_lift_moments(st, a["N"], a["points"], a["V"], a["views"], a["masks"], a["orients"], a["confs"], a["tab"], a["prev"],
                                  a["s2"], a["min_conf"], a["M"], a["wsum"], a["count"])
    bad = [dict(V=0), dict(V=4097), dict(min_conf=-1), dict(min_conf=256), dict(s2=0.0), dict(s2=-1.0), dict(s2=float("inf")),
           dict(s2=float("nan")), dict(N=-1)]
    bad += [{k: None} for k in ("points", "views", "masks", "orients", "confs", "tab", "M", "wsum", "count")]
    for change in bad:
        assert moments(**change) != 0, change
        assert L.hgs_last_error().startswith(b"hgs_lift_moments")
    for args in ((8, rt.ptr(M), rt.ptr(count), 1, rt.ptr(d), rt.ptr(coh)), (8, rt.ptr(M), rt.ptr(count), 0, rt.ptr(d), rt.ptr(coh)),
                 (8, None, rt.ptr(count), 2, rt.ptr(d), rt.ptr(coh)), (8, rt.ptr(M), None, 2, rt.ptr(d), rt.ptr(coh)),
                 (8, rt.ptr(M), rt.ptr(count), 2, None, rt.ptr(coh)), (8, rt.ptr(M), rt.ptr(count), 2, rt.ptr(d), None),
                 (-1, rt.ptr(M), rt.ptr(count), 2, rt.ptr(d), rt.ptr(coh))):
        assert L.hgs_lift_solve(st, *args) != 0, args
    torch.cuda.synchronize()
    assert not M.any() and not wsum.any() and not count.any() and not d.any() and not coh.any()      # nothing was launched
    assert moments(s2=0.0, prev=None) == 0 and moments(N=0, points=None, M=None) == 0                # (s2 only matters with prev)
    # the wrappers raise
    with pytest.raises(rt.HgsError):
        lift.moments_device(dev, packed, p, 0.0)
    with pytest.raises(rt.HgsError):
        lift.moments_device(dev, packed, min_conf=256)
    with pytest.raises(rt.HgsError):
        lift.solve_device(M, count, 1)
    with pytest.raises(rt.HgsError):
        lift.moments_device(dev.cpu(), packed)
    with pytest.raises(rt.HgsError):
        lift.moments_device(dev.float(), packed)
    with pytest.raises(rt.HgsError):
        lift.moments_device(dev, packed, p[:4].contiguous(), 0.03)
    for name in ("orients_dev", "confs_dev"):                    # a plane buffer shorter than offset + W*H
        short = lift.Packed(packed.carve, packed.orients_dev, packed.confs_dev, packed.tab_dev)
        setattr(short, name, getattr(packed, name)[:-1].contiguous())
        with pytest.raises(rt.HgsError, match=name[:-4]):
            lift.moments_device(dev, short)
    with pytest.raises(rt.HgsError, match="mask"):
        lift.moments_device(dev, lift.Packed(carve.Packed(packed.carve.records, packed.carve.views_dev, packed.carve.masks_dev[:-1].contiguous()),
                                             packed.orients_dev, packed.confs_dev, packed.tab_dev))
    with pytest.raises(rt.HgsError, match="table"):
        lift.moments_device(dev, lift.Packed(packed.carve, packed.orients_dev, packed.confs_dev, packed.tab_dev[:255].contiguous()))
    with pytest.raises(rt.HgsError):
        lift.moments_device(dev, lift.Packed(packed.carve, packed.orients_dev.cpu(), packed.confs_dev, packed.tab_dev))


# ---- 5. the driver on both devices ---------------------------------------------------------------------------------------------
def _scene(root, smooth):
    views, masks, images, _ = CC.build_scene(root)
    if smooth:
        orients, confs, _ = LC.smooth_orientations(root, views)
    else:
        orients, confs = LC.write_orientations(root, views)
    return views, masks, orients, confs


def test_driver_directions_agree_on_both_devices(tmp_path):
    import init_cloud
    from data.dataset_readers import fetchPly
    from utils import lift
    bins, normals = {}, {}
    for device in ("cuda", "cpu"):
        src = str(tmp_path / device)
        views, masks, orients, confs = _scene(src, smooth=False)
        n = init_cloud.main(["-s", src, "--device", device, "--grid", "24", "--min_views", "6", "--min_percent", "100", "--directions"])
        sparse = os.path.join(src, "sparse", "0")
        with open(os.path.join(sparse, "points3D.bin"), "rb") as fh:
            bins[device] = fh.read()
        normals[device] = fetchPly(os.path.join(sparse, "points3D.ply")).normals.astype(np.float64)
        assert n > 100 and normals[device].shape == (n, 3)
    assert bins["cuda"] == bins["cpu"]
    xyz = CC.read_points(os.path.join(str(tmp_path / "cpu"), "sparse", "0", "points3D.bin"))[0]
    prev = lift.lift_directions(xyz, views, masks, orients, confs, rounds=2)[0]
    M = lift.lift_moments(xyz, views, masks, orients, confs, prev, lift.sin2(10.0))[0]              # the last round's matrices
    zero = ~normals["cpu"].any(axis=1)
    assert np.array_equal(zero, ~normals["cuda"].any(axis=1)) and zero.sum() < len(zero) // 2
    tight = ~zero & (LC.relative_gap(M) >= 1e-6)
    # (the file holds float32: a stored vector is a unit vector to 6e-8 only, so the rule's dot product of unit vectors is taken of
    # the stored vectors renormalised in float64 -- the same angle, and still the bound of the solve test)
    unit = {k: v[tight] / np.linalg.norm(v[tight], axis=1, keepdims=True) for k, v in normals.items()}
    dot = np.abs((unit["cuda"] * unit["cpu"]).sum(axis=1))
    print(f"{int(tight.sum())} of {int((~zero).sum())} directions above the gap: max 1 - |dot| = {float((1.0 - dot).max()):.3e}")
    assert (~zero & ~tight).sum() <= 0.01 * (~zero).sum()
    assert (1.0 - dot).max() <= 1e-12
    assert np.allclose(np.linalg.norm(normals["cuda"][~zero], axis=1), 1.0, rtol=0, atol=1e-6)      # (float32 in the file)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_directions_initialise_stage_one(tmp_path):
    import init_cloud
    from arguments import OptimizationParams
    from data.dataset_readers import fetchPly
    from scene import Scene
    from scene.gaussian_model import GaussianModel
    from simple_knn._C import distCUDA2
    from train import training_step
    src = str(tmp_path / "scene")
    _, _, _, _ = _scene(src, smooth=True)
    n = init_cloud.main(["-s", src, "--device", "cuda", "--grid", "24", "--min_views", "6", "--min_percent", "100", "--directions"])
    pcd = fetchPly(os.path.join(src, "sparse", "0", "points3D.ply"))
    has = torch.from_numpy(pcd.normals.any(axis=1)).cuda()
    assert int(has.sum()) > n // 2
    args = SimpleNamespace(source_path=src, model_path=str(tmp_path / "model"), images="images", sh_degree=0, resolution=-1,
                           data_device="cuda", eval=False, init_directions=True, direction_stretch=3.0)
    scene = Scene(args, shuffle=False)
    g = scene.gaussians
    assert g.get_xyz.shape[0] == n
    want = torch.from_numpy(pcd.normals).cuda()
    got = g.get_orientation.detach()
    err = torch.minimum((got - want).abs().amax(dim=1), (got + want).abs().amax(dim=1))
    print(f"{int(has.sum())} of {n} Gaussians start along a lifted direction; largest deviation {float(err[has].max()):.2e}")
    assert float(err[has].max()) <= 1e-5
    assert (g.get_scaling[has, 0] > g.get_scaling[has, 1]).all()
    # without the option: the parent's parameters, bit for bit (restated here), whether through the default or through False
    plain, off = GaussianModel(0, scene.cameras_extent, device="cuda"), GaussianModel(0, scene.cameras_extent, device="cuda")
    plain.create_from_pcd(pcd)
    off.create_from_pcd(pcd, init_directions=False, direction_stretch=7.0)
    pts = torch.tensor(np.asarray(pcd.points)).float().cuda()
    scales = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(pts), 0.0000001)))[..., None].repeat(1, 3)
    rots = torch.zeros((n, 4), device="cuda")
    rots[:, 0] = 1
    for m in (plain, off):
        assert torch.equal(m._scaling, scales) and torch.equal(m._rotation, rots) and torch.equal(m._xyz, pts)
    for _, attr in GaussianModel._PARAM_ATTRS:
        assert torch.equal(getattr(plain, attr), getattr(off, attr))
        if attr not in ("_scaling", "_rotation"):
            assert torch.equal(getattr(plain, attr), getattr(g, attr))
    assert torch.equal(g._scaling[~has], scales[~has]) and torch.equal(g._rotation[~has], rots[~has])
    # one iteration of the existing loop
    opt = OptimizationParams()
    opt.enable_topology = False
    g.training_setup(opt)
    cams = scene.getCameras()
    loss = training_step(g, cams[0], opt, torch.zeros(3, device="cuda"), 1, extent=scene.cameras_extent)[0]
    assert np.isfinite(float(loss))
