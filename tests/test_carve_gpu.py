"""hgs_carve_grid, hgs_carve_shell and hgs_carve_votes (csrc/hgs_carve.hip) against the numpy path of utils/carve.py: equal arrays, no
tolerance, at the smallest shapes where the kernels can go wrong -- row lengths around the 64-lane wavefront and the 64 x 4 brick,
one voxel, several z slices, 1 / 3 / 7 views of two sizes, every corner of the keep rule, sparse and dense masks so that the view
loop is left early in both directions -- and the init_cloud.py driver, whose file is the same on both devices."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import carve_cases as CC

pytestmark = pytest.mark.gpu


def _grid_case(nx, ny, nz):
    """Origin and voxel size: the grid is centred near the ring's centre and, where it is long, reaches past the cameras (radius 3), so
    that some voxels are in no frame."""
    h = 8.0 / max(nx, 16)
    return np.array([0.05 - 0.5 * h * nx, -0.03 - 0.5 * h * ny, 0.3 - 0.5 * h * nz]), h


@pytest.fixture(scope="module")
def packed_views():
    """{(V, density): (views, masks, Packed)}, uploaded once."""
    from utils import carve
    out = {}
    for V in (1, 3, 7):
        views = CC.ring_views(V)
        for density in (0.3, 0.9):
            masks = CC.random_masks(views, density, seed=V)
            out[V, density] = (views, masks, carve.pack(views, masks, None, "cuda"))
    return out


@pytest.mark.parametrize("ny,nz", [(1, 1), (3, 2), (5, 7)])
@pytest.mark.parametrize("nx", [1, 2, 63, 64, 65, 130, 257])
def test_grid_and_shell_equal_the_numpy_path(packed_views, nx, ny, nz):
    from utils import carve
    origin, h = _grid_case(nx, ny, nz)
    dims = (nx, ny, nz)
    zeros = ones = 0
    for (V, density), (views, masks, packed) in packed_views.items():
        c = carve.centres(origin, h, dims)
        Z, Y, X = np.meshgrid(c[2], c[1], c[0], indexing="ij")
        seen, hits = carve.votes_numpy(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1), views, masks)
        for min_views in (1, V, V + 1):
            for min_percent in (0, 50, 100):
                want = carve.keep(seen, hits, min_views, min_percent).reshape(nz, ny, nx).astype(np.uint8)
                if (min_views, min_percent) in ((1, 50), (V, 100)):          # (the same thing through the public numpy entry point)
                    assert np.array_equal(want, carve.grid_numpy(origin, h, dims, views, masks, min_views, min_percent))
                occ = carve.grid_device(origin, h, dims, packed, min_views, min_percent)
                assert occ.shape == (nz, ny, nx) and occ.dtype == torch.uint8
                assert np.array_equal(occ.cpu().numpy(), want), (V, density, min_views, min_percent)
                assert np.array_equal(carve.shell_device(occ).cpu().numpy(), carve.shell_numpy(want)), (V, density, min_views, min_percent)
                if min_views == V + 1:
                    assert not want.any()                                    # the rule forbids a kept voxel
                else:
                    zeros += int((want == 0).sum())
                    ones += int((want == 1).sum())
                    if nx >= 63 and ny > 1 and min_views == 1 and min_percent == 100:   # kept iff seen and hits == seen: density ** seen of them
                        assert want.any() and not want.all(), (V, density, min_views)
    assert zeros > 0 and ones > 0


def _vote_inputs():
    """Views (three ring views and the identity view of the border cases), masks, images and 1000 points: the border points, NaN / Inf
    points and points behind a camera first."""
    views = CC.ring_views(3) + [CC.identity_view(45, 31)]
    masks, images = CC.random_masks(views, 0.7, seed=5), CC.random_images(views, seed=6)
    border, _ = CC.border_points(45, 31)
    behind = np.array([[4.0, 0.0, 0.0], [0.0, 5.0, 0.2], [-6.0, 1.0, 0.3]])
    pts = np.concatenate([border, behind, CC.cloud(1000, seed=8)])[:1000]
    return views, masks, images, np.ascontiguousarray(pts)


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1000])
def test_votes_equal_the_numpy_path(N):
    from utils import carve
    views, masks, images, pts = _vote_inputs()
    pts = pts[:N]
    want = carve.votes_numpy(pts, views, masks, images)
    dev = torch.from_numpy(pts).cuda()
    got = carve.votes_device(dev, carve.pack(views, masks, images, "cuda"), with_rgb=True)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
    got2 = carve.votes_device(dev, carve.pack(views, masks, None, "cuda"))
    assert len(got2) == 2 and np.array_equal(got2[0].cpu().numpy(), want[0]) and np.array_equal(got2[1].cpu().numpy(), want[1])
    if N >= 63:
        border, seen_identity = CC.border_points(45, 31)
        only = carve.votes_device(dev[:len(border)].contiguous(), carve.pack(views[3:], masks[3:], None, "cuda"))[0]
        assert np.array_equal(only.cpu().numpy(), seen_identity)
        assert want[1].sum() > 0 and (want[0] < 4).any() and want[2].max() > 255
    # the host-array entry point
    host = carve.mask_votes(pts, views, masks, images, device="cuda")
    assert all(np.array_equal(a, b) for a, b in zip(host, want))


def test_early_exit_changes_nothing(packed_views):
    """occ is the keep rule applied to hgs_carve_votes' counts (which has no early exit) on the same centres."""
    from utils import carve
    dims = (130, 5, 7)
    origin, h = _grid_case(*dims)
    c = carve.centres(origin, h, dims)
    Z, Y, X = np.meshgrid(c[2], c[1], c[0], indexing="ij")
    pts = torch.from_numpy(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)).cuda()
    for (V, density), (views, masks, packed) in packed_views.items():
        seen, hits = carve.votes_device(pts, packed)
        for min_views in (1, 2, V):
            for min_percent in (0, 1, 34, 50, 67, 99, 100):
                occ = carve.grid_device(origin, h, dims, packed, min_views, min_percent)
                want = carve.keep(seen, hits, min_views, min_percent).reshape(7, 5, 130).to(torch.uint8)
                assert torch.equal(occ, want), (V, density, min_views, min_percent)


def test_repeatable_and_stream_independent(packed_views):
    from utils import carve
    views, masks, packed = packed_views[7, 0.3]
    dims = (130, 5, 7)
    origin, h = _grid_case(*dims)
    pts = torch.from_numpy(CC.cloud(1000, seed=1)).cuda()

    def run():
        occ = carve.grid_device(origin, h, dims, packed, 2, 50)
        return (occ, carve.shell_device(occ)) + carve.votes_device(pts, packed)
    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_dilate_device_equals_numpy():
    from utils import carve
    mask = CC.random_masks([CC.identity_view(45, 31)], 0.05, seed=2)[0]
    for r in (0, 1, 3):
        assert np.array_equal(carve.dilate(mask, r, device="cuda"), carve.dilate(mask, r))


def test_refusals(packed_views):
    import hgs_runtime as rt
    from utils import carve
    views, masks, packed = packed_views[3, 0.3]
    with pytest.raises(rt.HgsError):                                          # a host tensor
        carve.votes_device(torch.zeros((4, 3), dtype=torch.float64), packed)
    with pytest.raises(rt.HgsError):
        carve.shell_device(torch.ones((2, 2, 2), dtype=torch.uint8))
    with pytest.raises(rt.HgsError):
        carve.votes_device(torch.zeros((4, 3), dtype=torch.float32, device="cuda"), packed)
    short = carve.Packed(packed.records, packed.views_dev, packed.masks_dev[:-1].contiguous())
    with pytest.raises(rt.HgsError, match="mask"):                            # a mask buffer shorter than offset + W*H
        carve.grid_device(np.zeros(3), 1.0, (2, 2, 2), short, 1, 50)
    with pytest.raises(rt.HgsError, match="mask"):
        carve.votes_device(torch.zeros((4, 3), dtype=torch.float64, device="cuda"), short)
    host = carve.Packed(packed.records, packed.views_dev, packed.masks_dev.cpu())
    with pytest.raises(rt.HgsError):
        carve.grid_device(np.zeros(3), 1.0, (2, 2, 2), host, 1, 50)
    for dims in ((1025, 1, 1), (1, 1025, 1), (1, 1, 0)):
        with pytest.raises(rt.HgsError, match="1 to 1024"):
            carve.grid_device(np.zeros(3), 1.0, dims, packed, 1, 50)
    with pytest.raises(rt.HgsError):
        carve.grid_device(np.zeros(3), 1.0, (2, 2, 2), packed, 0, 50)
    # the library refuses the same by itself
    L = rt.lib()
    o = np.zeros(3)
    occ = torch.zeros(8, dtype=torch.uint8, device="cuda")
    assert L.hgs_carve_grid(rt.current_stream(), o.ctypes.data, 1.0, 1025, 1, 1, 3, rt.ptr(packed.views_dev), rt.ptr(packed.masks_dev), 1,
                            50, rt.ptr(occ)) != 0
    assert b"1025" in L.hgs_last_error()
    assert L.hgs_carve_grid(rt.current_stream(), o.ctypes.data, 1.0, 2, 2, 2, 4097, rt.ptr(packed.views_dev), rt.ptr(packed.masks_dev), 1,
                            50, rt.ptr(occ)) != 0


@pytest.mark.parametrize("mode,extra", [("hull", ()), ("both", ("--dilate", "1"))])
def test_driver_writes_the_same_file_on_both_devices(tmp_path, mode, extra):
    import init_cloud
    files = {}
    for device in ("cuda", "cpu"):
        src = str(tmp_path / device)
        CC.build_scene(src)
        n = init_cloud.main(["-s", src, "--mode", mode, "--device", device, "--grid", "48", "--min_views", "6", "--min_percent", "100", *extra])
        with open(os.path.join(src, "sparse", "0", "points3D.bin"), "rb") as fh:
            files[device] = fh.read()
        assert n > 100 and len(files[device]) == 8 + 51 * n
    assert files["cuda"] == files["cpu"]


def test_carved_cloud_starts_stage_one(tmp_path):
    """A capture synthesized on the GPU, carved, loaded and trained for 20 iterations.  Prints (does not assert: the capture's masks
    are 1-pixel lines, not silhouettes) the share of the ground-truth points, of those in frame in at least min_views views, whose
    voxel is in the hull before the shell."""
    import init_cloud
    from arguments import OptimizationParams
    from scene import Scene
    from tests.test_mesh_raster_gpu import _synth
    from train import training_step
    from utils import carve
    src = _synth(tmp_path, "cuda", W=160, H=120, cams=6, extra=("--use_gt_hair_verts",))
    n = init_cloud.main(["-s", str(src), "--mode", "hull", "--grid", "64", "--device", "cuda"])
    assert n > 0
    args = SimpleNamespace(source_path=str(src), model_path=str(tmp_path / "model"), images="images", sh_degree=0, resolution=-1,
                           data_device="cuda", eval=False)
    scene = Scene(args, shuffle=False)
    cams = scene.getCameras()
    assert scene.gaussians.get_xyz.shape[0] == n
    opt = OptimizationParams()
    opt.enable_topology = False
    scene.gaussians.training_setup(opt)
    bg = torch.zeros(3, device="cuda")
    losses = [float(training_step(scene.gaussians, cams[it % len(cams)], opt, bg, it, extent=scene.cameras_extent)[0])
              for it in range(1, 21)]
    assert np.isfinite(losses).all()
    # the recorded figure
    from PIL import Image as PILImage
    from data.capture import read_sparse
    cameras, images = read_sparse(os.path.join(str(src), "sparse", "0"))
    views = [carve.view_of(cameras[im.camera_id], im) for im in images.values()]
    masks = [np.asarray(PILImage.open(os.path.join(str(src), "masks", v.name)).convert("L")) for v in views]
    voter = init_cloud._Voter(views, masks, None, "cuda", 0)
    lo, hi, _, origin, h, dims, occ = init_cloud.hull_grid(voter, None, 64, 3, 50)
    gt = np.load(os.path.join(str(src), "hair_eval_data.npz"))["points"].astype(np.float64)
    seen, _ = voter.votes(gt, False)
    idx = np.floor((gt - origin) / h).astype(np.int64)
    inside = ((idx >= 0) & (idx < np.array(dims))).all(axis=1)
    idx = np.clip(idx, 0, np.array(dims) - 1)
    covered = inside & (occ[idx[:, 2], idx[:, 1], idx[:, 0]] != 0)
    framed = seen >= 3
    print(f"carved cloud: {n} points, grid {dims}, {int(occ.sum())} voxels kept; {int((covered & framed).sum())} of {int(framed.sum())} "
          f"ground-truth points in frame in >= 3 views lie in a kept voxel ({100.0 * (covered & framed).sum() / max(1, framed.sum()):.1f} %); "
          f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
