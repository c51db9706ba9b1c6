"""utils/lift.py without a GPU: the numpy path against the scalar loop restatement of tests/lift_cases.py (exact), the geometry of the
convention (lifted lines against the true ones, with nothing free but the byte's quantisation step), the robust rounds, the degenerate
inputs, direction_init, the init_cloud.py --directions driver on --device cpu, and the binding."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from tests import carve_cases as CC
from tests import lift_cases as LC


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. equality with the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("V", [1, 3, 5])
def test_numpy_path_equals_the_restatement(V, with_prev):
    from utils import lift
    views = LC.equality_views(V)
    masks, orients, confs = LC.random_planes(views, seed=V)
    pts = LC.equality_points(120)
    prev = LC.unit_prev(len(pts)) if with_prev else None
    s2 = lift.sin2(10.0)
    for min_conf in (0, 1, 100):
        got = lift.lift_moments(pts, views, masks, orients, confs, prev, s2, min_conf)
        want = LC.moments_loop(pts, views, masks, orients, confs, lift.table(), prev, s2, min_conf)
        assert got[0].dtype == got[1].dtype == np.float64 and got[2].dtype == np.int32
        assert all(_bits(g, w) for g, w in zip(got, want)), (V, with_prev, min_conf)
        assert np.isfinite(got[0]).all() and 0 < got[2].sum() and (got[2] < V).any()
    if with_prev:                                                # the re-weighting changes the sums, except where prev is zero
        plain = lift.lift_moments(pts, views, masks, orients, confs, None, s2, 1)
        robust = lift.lift_moments(pts, views, masks, orients, confs, prev, s2, 1)
        zero = ~prev.any(axis=1)
        assert _bits(plain[0][zero], robust[0][zero]) and not _bits(plain[0], robust[0])
        assert (robust[1] <= plain[1]).all()


def test_table_is_the_loaders_angle():
    from utils import lift
    tab = lift.table()
    assert tab.shape == (256, 2) and tab.dtype == np.float64
    assert tab[0].tolist() == [0.0, 1.0] and abs(tab[255, 0]) < 1e-15 and tab[255, 1] == -1.0
    o = 64
    assert tab[o, 0] == np.sin(o * np.pi / 255) and tab[o, 1] == np.cos(o * np.pi / 255)


# ---- 2. geometry -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    views, pts, truth = LC.rig(8, 500, seed=0)
    orient, inside = LC.image_angle_bytes(views, pts, truth)
    assert inside.all()
    return views, pts, truth, orient


def _lift_samples(views, pts, orient, tab=None, rounds=0, sigma_deg=10.0):
    """lift_directions through the planes-free entry point (every view used, confidence 255); `tab` replaces the contract's table."""
    from utils import lift
    used, conf = np.ones(orient.shape, bool), np.full(orient.shape, 255, np.uint8)
    original = lift.table
    if tab is not None:
        lift.table = lambda: tab
    try:
        prev, M0 = None, None
        for _ in range(rounds + 1):
            M, _, count = lift.moments_from_samples(pts, views, used, orient, conf, prev, lift.sin2(sigma_deg))
            M0 = M if M0 is None else M0
            prev, coherence = lift.solve_numpy(M, count)
    finally:
        lift.table = original
    return prev, coherence, M0


def test_lifted_lines_are_the_true_lines(geometry):
    from utils import lift
    views, pts, truth, orient = geometry
    d, coherence, M = _lift_samples(views, pts, orient)
    gap = LC.relative_gap(M)
    err = LC.angle_deg(d, truth)
    print(f"smallest relative eigengap {gap.min():.4f}; error max {err.max():.3f} deg, median {np.median(err):.3f} deg (step {LC.STEP_DEG:.3f})")
    assert gap.min() >= 0.05                                     # a condition on the inputs
    assert err.max() <= LC.STEP_DEG
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0) and (coherence > 0.9).all()
    top = d[np.arange(len(d)), np.argmax(np.abs(d), axis=1)]
    assert (top > 0).all()                                       # the sign rule
    tab = lift.table()
    mirrored = np.stack([-tab[:, 0], tab[:, 1]], axis=1)
    swapped = np.ascontiguousarray(tab[:, ::-1])
    for name, wrong in (("mirrored", mirrored), ("swapped", swapped)):
        bad = np.median(LC.angle_deg(_lift_samples(views, pts, orient, wrong)[0], truth))
        print(f"{name} table: median error {bad:.2f} deg")
        assert bad > np.median(err)


# ---- 3. robust rounds ----------------------------------------------------------------------------------------------------------
def test_rounds_do_not_raise_the_error_and_beat_least_squares():
    views, pts, truth = LC.rig(16, 500, seed=1)
    orient, inside = LC.image_angle_bytes(views, pts, truth)
    assert inside.all()
    rng = np.random.default_rng(2)
    noisy = np.where(rng.random(orient.shape) < 0.5, rng.integers(0, 256, orient.shape), orient).astype(np.uint8)
    med = [float(np.median(LC.angle_deg(_lift_samples(views, pts, noisy, rounds=r)[0], truth))) for r in range(4)]
    print("median error per round (deg):", ", ".join(f"{m:.2f}" for m in med))
    assert all(b <= a for a, b in zip(med, med[1:]))
    assert med[3] < med[0]


def test_lift_directions_is_the_loop_of_its_parts():
    from utils import lift
    views = LC.equality_views(5)
    masks, orients, confs = LC.random_planes(views, seed=9, density=0.95)
    pts = LC.equality_points(200)
    M, _, count = lift.lift_moments(pts, views, masks, orients, confs)
    d0, c0 = lift.lift_solve(M, count)
    got = lift.lift_directions(pts, views, masks, orients, confs, rounds=0)
    assert _bits(got[0], d0) and _bits(got[1], c0) and _bits(got[2], count)
    M1, _, count1 = lift.lift_moments(pts, views, masks, orients, confs, d0, lift.sin2(10.0))
    d1, c1 = lift.lift_solve(M1, count1)
    got = lift.lift_directions(pts, views, masks, orients, confs, rounds=1, sigma_deg=10.0)
    assert _bits(got[0], d1) and _bits(got[1], c1)
    assert d0.any(axis=1).sum() > 20
    for bad in (dict(rounds=-1), dict(sigma_deg=0.0), dict(min_conf=256), dict(min_views=1), dict(device="cpu")):
        with pytest.raises(ValueError):
            lift.lift_directions(pts, views, masks, orients, confs, **bad)
    with pytest.raises(ValueError):
        lift.lift_moments(pts, views, masks, orients[:-1], confs)
    with pytest.raises(ValueError):
        lift.lift_moments(pts, views, masks, orients, [c.astype(np.float32) for c in confs])


# ---- 4. degenerate inputs ---------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    from utils import lift
    W, H = 9, 7
    v = CC.identity_view(W, H)
    full = np.full((H, W), 255, np.uint8)
    plane = lambda value: np.full((H, W), value, np.uint8)       # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # nothing below may warn
        # count 0 and a single view (rank 1): no direction
        d, coh = lift.lift_solve(np.zeros((2, 6)), np.array([0, 5], np.int32))
        assert not d.any() and not coh.any()
        pt = np.array([[2.5, 3.5, 1.0]])
        M, wsum, count = lift.lift_moments(pt, [v], [full], [plane(40)], [full])
        assert count.tolist() == [1] and wsum.tolist() == [1.0] and M.any()
        assert not lift.lift_solve(M, count)[0].any()
        # two views with the same plane: count 2, still rank 1 -- zero or a unit vector, finite either way
        M, _, count = lift.lift_moments(pt, [v, v], [full] * 2, [plane(40)] * 2, [full] * 2)
        d, coh = lift.lift_solve(M, count)
        assert count.tolist() == [2] and np.isfinite(d).all() and np.isfinite(coh).all()
        assert np.linalg.norm(d[0]) == 0.0 or abs(np.linalg.norm(d[0]) - 1.0) < 1e-12
        # zc <= 0 everywhere, the borders of the frame, NaN and Inf
        pts, seen = CC.border_points(W, H)
        M, wsum, count = lift.lift_moments(pts, [v], [full], [plane(40)], [full])
        assert np.array_equal(count, seen) and np.isfinite(M).all() and np.array_equal(wsum, seen.astype(np.float64))
        assert not M[seen == 0].any()
        d, coh, count = lift.lift_directions(pts, [v, v], [full] * 2, [plane(40), plane(90)], [full] * 2)
        assert np.isfinite(d).all() and np.isfinite(coh).all() and np.array_equal(count, 2 * seen) and not d[seen == 0].any()
        assert np.allclose(np.linalg.norm(d[seen == 1], axis=1), 1.0)
        # conf below min_conf; min_conf = 0 admits a zero confidence with a zero weight
        pt = np.array([[2.5, 3.5, 1.0]])
        assert lift.lift_moments(pt, [v], [full], [plane(40)], [plane(9)], min_conf=10)[2].tolist() == [0]
        assert lift.lift_moments(pt, [v], [full], [plane(40)], [plane(10)], min_conf=10)[2].tolist() == [1]
        M, wsum, count = lift.lift_moments(pt, [v], [full], [plane(40)], [plane(0)], min_conf=0)
        assert count.tolist() == [1] and wsum.tolist() == [0.0] and not M.any()
        assert lift.lift_moments(pt, [v], [plane(0)], [plane(40)], [full])[2].tolist() == [0]          # off the mask
        # orient 0 and 255 are the same line
        other = CC.ring_views(2)[1]
        planes = lambda value: [plane(value), np.full((other.H, other.W), 77, np.uint8)]                 # noqa: E731
        ms = [full, np.full((other.H, other.W), 255, np.uint8)]
        near = np.array([[0.05, 0.02, 1.0]])
        d0 = lift.lift_directions(near, [v, other], ms, planes(0), ms)[0]
        d255 = lift.lift_directions(near, [v, other], ms, planes(255), ms)[0]
        assert abs(np.linalg.norm(d0[0]) - 1.0) < 1e-12 and LC.angle_deg(d0, d255)[0] < 1e-6
        # prev = 0 takes the plain weight, bit for bit
        views = CC.ring_views(3)
        masks, orients, confs = LC.random_planes(views, seed=1, density=1.0)
        cloud = CC.cloud(50, seed=2, spread=0.3)
        plain = lift.lift_moments(cloud, views, masks, orients, confs)
        zero = lift.lift_moments(cloud, views, masks, orients, confs, np.zeros((50, 3)), lift.sin2(10.0))
        assert all(_bits(a, b) for a, b in zip(plain, zero)) and plain[2].sum() > 0
        # a matrix that is not finite gives no direction
        bad = np.array([[1.0, 0, 0, np.inf, 0, 1.0], [np.nan, 0, 0, 1.0, 0, 1.0]])
        d, coh = lift.lift_solve(bad, np.array([3, 3], np.int32))
        assert not d.any() and not coh.any()
    assert lift.lift_moments(np.zeros((0, 3)), [v], [full], [plane(1)], [full])[0].shape == (0, 6)
    assert lift.lift_solve(np.zeros((0, 6)), np.zeros(0, np.int32))[0].shape == (0, 3)


def test_solve_takes_the_smallest_eigenvector_with_the_sign_rule():
    from utils import lift
    # diag(3, 1, 2) rotated: the eigenvector of 1 is known
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    A = Q @ np.diag([3.0, 1.0, 2.0]) @ Q.T
    M = np.array([[A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]]])
    d, coh = lift.lift_solve(M, np.array([2], np.int32))
    assert LC.angle_deg(d, Q[:, 1][None])[0] < 1e-6 and d[0, np.argmax(np.abs(d[0]))] > 0
    assert abs(coh[0] - (2.0 - 1.0) / (2.0 + 1.0)) < 1e-12
    assert not lift.lift_solve(M, np.array([2], np.int32), min_views=3)[0].any()
    tie = np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 1.0 + 1e-3]])      # l0 = l1: any vector of the plane, coherence 0
    d, coh = lift.lift_solve(tie, np.array([4], np.int32))
    assert abs(np.linalg.norm(d[0]) - 1.0) < 1e-12 and abs(coh[0]) < 1e-12


# ---- 5. direction_init -------------------------------------------------------------------------------------------------------
def test_direction_init():
    import torch
    from scene.gaussian_model import direction_init
    from utils.transform import build_rotation
    rng = np.random.default_rng(4)
    n = 64
    normals = rng.normal(size=(n, 3)) * rng.uniform(0.1, 5.0, size=(n, 1))
    normals[::5] = 0.0
    normals[1] = (-1.0, 0.0, 0.0)
    normals[2] = (1.0, 0.0, 0.0)
    normals[3] = (-1e-9, 1.0, 0.0)
    dist2 = torch.tensor(rng.uniform(1e-6, 1e-2, n), dtype=torch.float32)
    scales, rots = direction_init(dist2, torch.tensor(normals, dtype=torch.float32), 3.0)
    assert scales.shape == (n, 3) and rots.shape == (n, 4) and scales.dtype == rots.dtype == torch.float32
    assert torch.isfinite(scales).all() and torch.isfinite(rots).all()
    has = torch.tensor(np.any(normals != 0, axis=1))
    d = torch.tensor(normals / np.maximum(np.linalg.norm(normals, axis=1, keepdims=True), 1e-300), dtype=torch.float32)
    axis = build_rotation(rots)[:, :, 0]
    err = torch.minimum((axis - d).abs().amax(dim=1), (axis + d).abs().amax(dim=1))
    assert float(err[has].max()) <= 1e-6
    assert (scales[has, 0] > scales[has, 1]).all() and torch.equal(scales[has, 1], scales[has, 2])
    assert torch.allclose(scales[has, 0] - scales[has, 1], torch.full((int(has.sum()),), float(np.log(3.0))), atol=1e-5)
    # zero-normal rows: exactly today's values
    default = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
    assert torch.equal(scales[~has], default[~has]) and torch.equal(scales[:, 1:], default[:, 1:])
    identity = torch.zeros((n, 4))
    identity[:, 0] = 1
    assert torch.equal(rots[~has], identity[~has])
    assert torch.allclose(rots.norm(dim=1), torch.ones(n), atol=1e-6)
    assert rots[1].tolist() == [1.0, 0.0, 0.0, 0.0] and rots[2].tolist() == [1.0, 0.0, 0.0, 0.0]      # d = (-1, 0, 0) is the line of e_x


def test_model_params_and_store_ply(tmp_path):
    from argparse import ArgumentParser
    from arguments import ModelParams
    from data.dataset_readers import fetchPly, storePly
    parser = ArgumentParser()
    mp = ModelParams(parser)
    assert mp.init_directions is False and mp.direction_stretch == 3.0
    args = parser.parse_args(["--init_directions", "--direction_stretch", "2.5"])
    assert args.init_directions is True and args.direction_stretch == 2.5
    rng = np.random.default_rng(0)
    xyz, rgb, nrm = rng.normal(size=(7, 3)), rng.integers(0, 256, (7, 3), dtype=np.uint8), rng.normal(size=(7, 3))
    a, b, c = (str(tmp_path / f"{k}.ply") for k in "abc")
    storePly(a, xyz, rgb)
    storePly(b, xyz, rgb, None)
    storePly(c, xyz, rgb, nrm)
    assert open(a, "rb").read() == open(b, "rb").read() and len(open(c, "rb").read()) == len(open(a, "rb").read())
    assert not fetchPly(a).normals.any()
    assert np.array_equal(fetchPly(c).normals, nrm.astype(np.float32)) and np.array_equal(fetchPly(c).points, fetchPly(a).points)


# ---- 6. driver -----------------------------------------------------------------------------------------------------------------
def _hull_args(extra=()):
    return ["--device", "cpu", "--grid", "24", "--min_views", "6", "--min_percent", "100", *extra]


def test_driver_writes_the_directions_and_the_loader_reads_them(tmp_path, capsys):
    import init_cloud
    from data.dataset_readers import fetchPly, readColmapSceneInfo
    from utils import lift
    src = str(tmp_path / "scene")
    views, masks, images, _ = CC.build_scene(src)
    orients, confs = LC.write_orientations(src, views)
    sparse = os.path.join(src, "sparse", "0")
    n = init_cloud.main(["-s", src, *_hull_args(["--directions"])])
    out = capsys.readouterr().out
    assert "directions:" in out and "median coherence" in out
    assert sorted(os.listdir(sparse)) == ["cameras.bin", "images.bin", "points3D.bin", "points3D.colmap.bin", "points3D.ply"]
    xyz, rgb, _ = CC.read_points(os.path.join(sparse, "points3D.bin"))
    d, coherence, count = lift.lift_directions(xyz, views, masks, orients, confs)
    assert n == len(xyz) and d.any(axis=1).sum() > n // 2
    pcd = fetchPly(os.path.join(sparse, "points3D.ply"))
    assert np.array_equal(pcd.normals, d.astype(np.float32))
    assert np.array_equal(pcd.points, xyz.astype(np.float32)) and np.array_equal(np.rint(pcd.colors * 255).astype(np.uint8), rgb)
    loaded = readColmapSceneInfo(src).point_cloud
    assert np.array_equal(loaded.normals, d.astype(np.float32)) and loaded.points.shape == (n, 3)
    # --min_coherence zeroes the directions below it; the knobs reach the lift
    init_cloud.main(["-s", src, *_hull_args(["--directions", "--overwrite", "--min_coherence", "0.5", "--rounds", "1", "--sigma_deg", "20",
                                             "--min_conf", "30"])])
    d1, c1, _ = lift.lift_directions(xyz, views, masks, orients, confs, rounds=1, sigma_deg=20.0, min_conf=30)
    want = np.where((c1 >= 0.5)[:, None], d1, 0.0)
    assert np.array_equal(fetchPly(os.path.join(sparse, "points3D.ply")).normals, want.astype(np.float32))
    assert 0 < want.any(axis=1).sum() < d1.any(axis=1).sum()
    # without the flag the folder is as before, and an earlier run's points3D.ply is gone
    init_cloud.main(["-s", src, *_hull_args(["--overwrite"])])
    assert sorted(os.listdir(sparse)) == ["cameras.bin", "images.bin", "points3D.bin", "points3D.colmap.bin"]


def test_driver_refuses_a_missing_or_misshapen_orientation_map(tmp_path):
    import init_cloud
    from PIL import Image as PILImage
    src = str(tmp_path / "scene")
    views, _, _, _ = CC.build_scene(src)
    LC.write_orientations(src, views, folder="maps")
    with pytest.raises(SystemExit, match="axis_0_orientation.png is missing"):                  # (the default folder does not exist)
        init_cloud.main(["-s", src, *_hull_args(["--directions"])])
    os.remove(os.path.join(src, "maps", "axis_2_confidence.png"))
    with pytest.raises(SystemExit, match="axis_2_confidence.png is missing"):
        init_cloud.main(["-s", src, *_hull_args(["--directions", "--orientations", "maps"])])
    PILImage.fromarray(np.zeros((10, 64), np.uint8)).save(os.path.join(src, "maps", "axis_2_confidence.png"))
    with pytest.raises(SystemExit, match="64 x 10"):
        init_cloud.main(["-s", src, *_hull_args(["--directions", "--orientations", "maps"])])
    with pytest.raises(SystemExit, match="--rounds"):
        init_cloud.main(["-s", src, *_hull_args(["--directions", "--orientations", "maps", "--rounds", "-1"])])
    sparse = os.path.join(src, "sparse", "0")                     # a refused run leaves the points where they were
    assert sorted(os.listdir(sparse)) == ["cameras.bin", "images.bin", "points3D.bin"]


# ---- 7. binding ------------------------------------------------------------------------------------------------------------------
def test_binding_loads():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15
    assert L.hgs_carve_view_bytes() == ctypes.sizeof(rt.CarveView) == 152
    for name, n_args in (("hgs_lift_moments", 15), ("hgs_lift_solve", 7)):
        assert hasattr(L, name) and len(rt.SIGNATURES[name][1]) == n_args
    assert callable(rt.lift_check)
