"""utils/carve.py without a GPU: the numpy path against the loop restatement of tests/carve_reference.py (exact), the border cases of
the in-frame test, the keep rule, a sphere carved from six axis views, the shell, the automatic bounds, the dilation, the points3D
writer, and the init_cloud.py driver on --device cpu."""
import ctypes
import os

import numpy as np
import pytest

from tests import carve_cases as CC
from tests import carve_reference as REF


# ---- equality with the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("dims", [(9, 5, 3), (1, 1, 1), (4, 1, 2)])
def test_numpy_path_equals_the_restatement(V, dims):
    from utils import carve
    views = CC.ring_views(V)
    masks, images = CC.random_masks(views, 0.6, seed=V), CC.random_images(views, seed=V)
    pts = CC.cloud(80, seed=3)
    seen, hits, rgb = carve.mask_votes(pts, views, masks, images)
    rseen, rhits, rrgb = REF.mask_votes(pts, views, masks, images)
    assert seen.dtype == hits.dtype == rgb.dtype == np.int32
    assert np.array_equal(seen, rseen) and np.array_equal(hits, rhits) and np.array_equal(rgb, rrgb)
    assert 0 < hits.sum() < seen.sum() and (seen < V).any()
    s2, h2 = carve.mask_votes(pts, views, masks)
    assert np.array_equal(s2, seen) and np.array_equal(h2, hits)
    origin, h = np.array([-1.1, -0.9, -0.7]), 2.0 / max(dims)
    for min_views, min_percent in ((1, 50), (V, 100), (1, 0)):
        occ = carve.carve_grid(origin, h, dims, views, masks, min_views, min_percent)
        assert occ.dtype == np.uint8 and occ.shape == dims[::-1]
        assert np.array_equal(occ, REF.carve_grid(origin, h, dims, views, masks, min_views, min_percent))
        assert np.array_equal(carve.shell(occ), REF.shell(occ))


# ---- border cases ----------------------------------------------------------------------------------------------------
def test_borders_of_the_frame_nan_inf_and_points_behind():
    from utils import carve
    W, H = 7, 5
    v = CC.identity_view(W, H)
    pts, want = CC.border_points(W, H)
    mask = np.full((H, W), 255, np.uint8)
    seen, hits = carve.mask_votes(pts, [v], [mask])
    assert np.array_equal(seen, want) and np.array_equal(hits, want)
    rseen, _ = REF.mask_votes(pts, [v], [mask])
    assert np.array_equal(rseen, want)
    # the pixel is (floor(v), floor(u)): (W - 1, H - 1) reads the last one
    mask2 = np.zeros((H, W), np.uint8)
    mask2[H - 1, W - 1] = 1                                      # a mask value of 1 counts as hair
    seen, hits = carve.mask_votes(np.array([[W - 1.0, H - 1.0, 1.0], [W - 0.5, H - 0.5, 1.0], [W - 2.0, H - 1.0, 1.0]]), [v], [mask2])
    assert seen.tolist() == [1, 1, 1] and hits.tolist() == [1, 1, 0]


def test_keep_rule_thresholds():
    from utils import carve
    V = 4
    views = [CC.identity_view(8, 8)] * V
    pt = np.array([[2.0, 3.0, 1.0]])
    for n_hit in range(V + 1):                                   # the point is seen by all V views and hit by n_hit of them
        masks = [np.full((8, 8), 1 if k < n_hit else 0, np.uint8) for k in range(V)]
        seen, hits = carve.mask_votes(pt, views, masks)
        assert (seen[0], hits[0]) == (V, n_hit)
        for min_views in (1, V, V + 1):
            for min_percent in (0, 50, 100):
                want = V >= min_views and 100 * n_hit >= min_percent * V
                occ = carve.carve_grid(np.array([1.5, 2.5, 0.5]), 1.0, (1, 1, 1), views, masks, min_views, min_percent)
                assert bool(occ[0, 0, 0]) == want == REF.kept(V, n_hit, min_views, min_percent), (n_hit, min_views, min_percent)
    assert bool(carve.keep(np.array([0]), np.array([0]), 1, 0)[0]) is False      # seen by nobody: never kept


def test_limits_are_refused():
    from utils import carve
    v = [CC.identity_view(4, 4)]
    m = [np.ones((4, 4), np.uint8)]
    for dims in ((1025, 1, 1), (1, 0, 1), (1, 1, 1025)):
        with pytest.raises(ValueError):
            carve.carve_grid(np.zeros(3), 1.0, dims, v, m, 1, 50)
    for rule in ((0, 50), (1, 101), (1, -1), (1.5, 50)):
        with pytest.raises(ValueError):
            carve.carve_grid(np.zeros(3), 1.0, (1, 1, 1), v, m, *rule)
    with pytest.raises(ValueError):
        carve.carve_grid(np.zeros(3), 1.0, (1, 1, 1), v * 4097, m * 4097, 1, 50)
    with pytest.raises(ValueError):
        carve.carve_grid(np.zeros(3), 1.0, (1, 1, 1), v, [np.ones((4, 5), np.uint8)], 1, 50)
    with pytest.raises(ValueError):
        carve.mask_votes(np.zeros((1, 3)), v, m, device="cpu")


# ---- sphere ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    r = 1.0
    views = CC.axis_views(10.0 * r)
    return r, views, [CC.sphere_mask(v, r) for v in views]


def test_sphere_mask_spans_twenty_pixels(sphere):
    r, views, masks = sphere
    assert all(int(m[32].astype(bool).sum()) in (40, 41) for m in masks)


@pytest.mark.parametrize("n", [24, 48, 65])
def test_sphere_is_carved(sphere, n):
    from utils import carve
    r, views, masks = sphere
    origin, h = np.full(3, -2.0 * r), 4.0 * r / n
    occ = carve.carve_grid(origin, h, (n, n, n), views, masks, 6, 100)
    c = carve.centres(origin, h, (n, n, n))
    Z, Y, X = np.meshgrid(c[2], c[1], c[0], indexing="ij")
    rad = np.sqrt(X * X + Y * Y + Z * Z)
    print(f"n = {n}: {int(occ.sum())} kept, largest kept radius {rad[occ == 1].max():.4f} r")
    assert occ[rad <= 0.9 * r].all()
    assert not occ[rad > 1.5 * r].any()
    assert occ.any() and not occ.all()


# ---- shell -----------------------------------------------------------------------------------------------------------
def test_shell_cases():
    from utils import carve
    assert np.array_equal(carve.shell(np.ones((1, 1, 1), np.uint8)), np.ones((1, 1, 1), np.uint8))
    lone = np.zeros((3, 4, 5), np.uint8)
    lone[1, 2, 3] = 1
    assert np.array_equal(carve.shell(lone), lone)
    want = np.ones((3, 3, 3), np.uint8)
    want[1, 1, 1] = 0
    assert np.array_equal(carve.shell(np.ones((3, 3, 3), np.uint8)), want)
    for shape in ((1, 1, 6), (1, 6, 1), (6, 1, 1)):
        assert carve.shell(np.ones(shape, np.uint8)).all()
    holed = np.ones((5, 5, 5), np.uint8)
    holed[2, 2, 2] = 0
    s = carve.shell(holed)
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        assert s[2 + d[0], 2 + d[1], 2 + d[2]] == 1
    assert s[2, 2, 2] == 0 and s[1, 1, 1] == 0 and s[1:4, 1:4, 1:4].sum() == 6 and s.sum() == 125 - 27 + 6
    assert np.array_equal(s, REF.shell(holed))


# ---- bounds, dilation, writer, selection -----------------------------------------------------------------------------
def test_auto_bounds_encloses_the_sphere(sphere):
    from utils import carve
    r, views, masks = sphere
    lo, hi = carve.auto_bounds(views, masks, 6, 100)
    cube_lo, side = carve.camera_cube(views)
    assert np.allclose(cube_lo, -10.0 * r) and np.isclose(side, 20.0 * r)
    hc = side / carve.COARSE
    assert (lo <= -r).all() and (hi >= r).all() and (hi - lo < 2 * 1.5 * r + 4 * hc).all()
    # padded by one coarse voxel: the box is the kept coarse voxels' box and one voxel more on every side
    occ = carve.carve_grid(cube_lo, hc, (64, 64, 64), views, masks, 6, 100)
    iz, iy, ix = np.nonzero(occ)
    assert np.allclose(lo, cube_lo + (np.array([ix.min(), iy.min(), iz.min()]) - 1) * hc)
    assert np.allclose(hi, cube_lo + (np.array([ix.max(), iy.max(), iz.max()]) + 2) * hc)
    origin, h, dims = carve.fine_grid(lo, hi, 32)
    assert np.array_equal(origin, lo) and h == (hi - lo).max() / 32 and max(dims) == 32 and min(dims) >= 1
    assert carve.fine_grid([0, 0, 0], [4, 1, 0], 8) == (pytest.approx(np.zeros(3)), 0.5, (8, 2, 1))
    with pytest.raises(ValueError, match="no voxel is consistent with the masks"):
        carve.auto_bounds(views, [np.zeros_like(m) for m in masks], 6, 100)


@pytest.mark.parametrize("r", [0, 1, 2, 5])
def test_dilate_equals_brute_force(r):
    from utils import carve
    rng = np.random.default_rng(r)
    mask = np.where(rng.random((9, 13)) < 0.1, rng.integers(1, 256, (9, 13)), 0).astype(np.uint8)
    assert np.array_equal(carve.dilate(mask, r), REF.dilate(mask, r))
    thin = np.zeros((1, 4), np.uint8)
    thin[0, 3] = 7
    assert np.array_equal(carve.dilate(thin, r), REF.dilate(thin, r))


def test_points_writer_equals_the_struct_writer(tmp_path):
    from data.colmap import Point3D, read_points3D_binary, write_points3D_arrays, write_points3D_binary
    rng = np.random.default_rng(0)
    n = 37
    xyz, rgb, err = rng.normal(size=(n, 3)), rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.uniform(0, 3, n)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    assert write_points3D_arrays(xyz, rgb, err, a) == n
    write_points3D_binary({i + 1: Point3D(id=i + 1, xyz=xyz[i], rgb=rgb[i], error=err[i], image_ids=[], point2D_idxs=[])
                           for i in range(n)}, b)
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) == 8 + 51 * n
    x, c, e = read_points3D_binary(a)
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb) and np.array_equal(e[:, 0], err)
    assert write_points3D_arrays(np.zeros((0, 3)), np.zeros((0, 3), np.uint8), np.zeros(0), a) == 0
    assert os.path.getsize(a) == 8 and read_points3D_binary(a)[0].shape == (0, 3)


def test_max_points_selection_and_colours():
    import init_cloud
    from utils.carve import select
    assert select(5, 5).tolist() == [0, 1, 2, 3, 4] and select(3, 10).tolist() == [0, 1, 2]
    for n, m in ((10, 3), (7, 6), (1000, 999), (200001, 200000)):
        got = select(n, m)
        assert got.tolist() == [(j * n) // m for j in range(m)] and len(set(got.tolist())) == m
    rgb = init_cloud.mean_colours(np.array([[10, 11, 12], [0, 0, 0], [255 * 3, 4, 5]]), np.array([4, 0, 3]))
    assert rgb.dtype == np.uint8 and rgb.tolist() == [[3, 3, 3], [128, 128, 128], [255, 1, 2]]


def test_struct_size_and_the_library_loads():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    assert L.hgs_carve_view_bytes() == ctypes.sizeof(rt.CarveView) == 152
    assert rt.CarveView.t.offset == 72 and rt.CarveView.W.offset == 128 and rt.CarveView.mask_offset.offset == 136
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15


# ---- driver ----------------------------------------------------------------------------------------------------------
def _hull_args(extra=()):
    return ["--device", "cpu", "--grid", "24", "--min_views", "6", "--min_percent", "100", *extra]


def test_driver_hull_files_backup_and_loader(tmp_path, capsys):
    import init_cloud
    from data.dataset_readers import readColmapSceneInfo
    src = str(tmp_path / "scene")
    views, masks, images, (xyz0, rgb0, err0) = CC.build_scene(src)
    sparse = os.path.join(src, "sparse", "0")
    original = open(os.path.join(sparse, "points3D.bin"), "rb").read()
    assert readColmapSceneInfo(src).point_cloud.points.shape[0] == 60           # (writes the loader's points3D.ply)
    assert os.path.exists(os.path.join(sparse, "points3D.ply"))
    n = init_cloud.main(["-s", src, *_hull_args()])
    out = capsys.readouterr().out
    assert "grid" in out and "voxel size" in out and "bounds (automatic)" in out and f"{n} written" in out
    assert not os.path.exists(os.path.join(sparse, "points3D.ply"))
    assert open(os.path.join(sparse, "points3D.colmap.bin"), "rb").read() == original
    assert sorted(os.listdir(sparse)) == ["cameras.bin", "images.bin", "points3D.bin", "points3D.colmap.bin"]
    xyz, rgb, err = CC.read_points(os.path.join(sparse, "points3D.bin"))
    assert n == xyz.shape[0] > 100 and (err == 0).all()
    rad = np.linalg.norm(xyz, axis=1)
    assert rad.min() > 0.7 and rad.max() < 1.5                                   # a shell around the unit sphere
    # the colours are the rounded means of mask_votes' sums
    from utils import carve
    _, hits, rgb_sum = carve.mask_votes(xyz, views, masks, images)
    assert (hits == 6).all() and np.array_equal(rgb, (rgb_sum + 3) // 6)
    assert readColmapSceneInfo(src).point_cloud.points.shape[0] == n
    # a second run is refused; with --overwrite it replaces the result and leaves the backup alone
    with pytest.raises(SystemExit, match="--overwrite"):
        init_cloud.main(["-s", src, *_hull_args()])
    n2 = init_cloud.main(["-s", src, *_hull_args(["--overwrite", "--no_shell", "--max_points", "50"])])
    assert n2 == 50 and open(os.path.join(sparse, "points3D.colmap.bin"), "rb").read() == original
    assert not os.path.exists(os.path.join(sparse, "points3D.ply"))
    assert CC.read_points(os.path.join(sparse, "points3D.bin"))[0].shape == (50, 3)


def test_driver_filter_and_both(tmp_path):
    import init_cloud
    from utils import carve
    src = str(tmp_path / "scene")
    views, masks, images, (xyz0, rgb0, err0) = CC.build_scene(src, text_points=True)
    sparse = os.path.join(src, "sparse", "0")
    seen, hits = carve.mask_votes(xyz0, views, masks)
    k = carve.keep(seen, hits, 6, 100)
    assert 5 < k.sum() < 55
    n = init_cloud.main(["-s", src, "--mode", "filter", *_hull_args()])
    assert n == int(k.sum()) and os.path.exists(os.path.join(sparse, "points3D.colmap.txt"))
    assert not os.path.exists(os.path.join(sparse, "points3D.txt"))
    xyz, rgb, err = CC.read_points(os.path.join(sparse, "points3D.bin"))
    assert np.array_equal(xyz, xyz0[k]) and np.array_equal(rgb, rgb0[k]) and np.array_equal(err[:, 0], err0[k])
    nb = init_cloud.main(["-s", src, "--mode", "both", "--overwrite", *_hull_args()])      # (reads the points from the backup)
    both = CC.read_points(os.path.join(sparse, "points3D.bin"))
    nh = init_cloud.main(["-s", src, "--mode", "hull", "--overwrite", *_hull_args()])
    hull = CC.read_points(os.path.join(sparse, "points3D.bin"))
    assert nb == n + nh
    for i, own in enumerate((xyz0[k], rgb0[k], err0[k][:, None])):
        assert np.array_equal(both[i], np.concatenate([own, hull[i]]))
    # --bounds replaces the search; --dilate widens the masks
    nd = init_cloud.main(["-s", src, "--overwrite", *_hull_args(["--bounds", "-2", "-2", "-2", "2", "2", "2", "--dilate", "2"])])
    n0 = init_cloud.main(["-s", src, "--overwrite", *_hull_args(["--bounds", "-2", "-2", "-2", "2", "2", "2"])])
    assert nd > n0 > 0


def test_driver_refusals(tmp_path):
    import init_cloud
    a, b, c = str(tmp_path / "opencv"), str(tmp_path / "nomask"), str(tmp_path / "nomasks")
    CC.build_scene(a, model="OPENCV")
    with pytest.raises(SystemExit, match="OPENCV.*undistort.py"):
        init_cloud.main(["-s", a, *_hull_args()])
    CC.build_scene(b, model="SIMPLE_PINHOLE")
    os.remove(os.path.join(b, "masks", "axis_3.png"))
    with pytest.raises(SystemExit, match="axis_3.png is missing"):
        init_cloud.main(["-s", b, *_hull_args()])
    from PIL import Image as PILImage
    PILImage.fromarray(np.zeros((10, 64), np.uint8)).save(os.path.join(b, "masks", "axis_3.png"))
    with pytest.raises(SystemExit, match="64 x 10"):
        init_cloud.main(["-s", b, *_hull_args()])
    CC.build_scene(c)
    for f in os.listdir(os.path.join(c, "masks")):
        os.remove(os.path.join(c, "masks", f))
    os.rmdir(os.path.join(c, "masks"))
    with pytest.raises(SystemExit, match="no masks/"):
        init_cloud.main(["-s", c, *_hull_args()])
    for scene in (a, b, c):                                       # a refused run leaves the points where they were
        assert os.path.exists(os.path.join(scene, "sparse", "0", "points3D.bin"))
        assert not os.path.exists(os.path.join(scene, "sparse", "0", "points3D.colmap.bin"))
