"""hgs_undistort_images (csrc/hgs_undistort.hip) against the numpy path of utils/undistort.py: the bytes and the validity plane are
equal, at the smallest shapes where the kernel can go wrong -- output widths around the per-lane run of 4 pixels and the 64-lane
wavefront, one row and odd row counts, one and three images, 1 / 3 / 4 channels on rows of odd length, every model, both modes,
with and without the validity plane, a principal point far outside the view -- and on one 640 x 480 image per model."""
import os

import numpy as np
import pytest
import torch

from tests import undistort_cases as UC

pytestmark = pytest.mark.gpu

WS, HS = 45, 31            # the small source: rows of 45, 135 and 180 bytes


def _device(images, cam, out_cam, mode, want_valid=True):
    from utils.undistort import undistort_device
    out, valid = undistort_device(torch.from_numpy(images).cuda(), cam, out_cam, mode, want_valid=want_valid)
    return out.cpu().numpy(), (valid.cpu().numpy() if want_valid else None)


def _images(N, C, mode, seed):
    if mode == "bilinear":
        return UC.noise(N, HS, WS, C, seed=seed)
    return np.ascontiguousarray(np.repeat(UC.binary_masks(N, HS, WS, seed=seed), C, axis=3))


@pytest.mark.parametrize("Wd,Hd", [(1, 1), (3, 5), (4, 7), (5, 1), (63, 3), (64, 5), (65, 9), (257, 3)])
def test_kernel_equals_numpy_path_at_small_shapes(Wd, Hd):
    """Every model x C x mode x N in {1, 3} (three different images) x validity plane given / NULL.  The output camera looks a little
    wider than the source, so that the outermost pixels are invalid."""
    from utils.undistort import undistort_numpy
    n_invalid = n_valid = 0
    for model in UC.MODELS:
        cam = UC.camera(model, WS, HS)
        out_cam = UC.pinhole(Wd, Hd, 0.8 * 36.0 * Wd / WS, 0.8 * 36.0 * Hd / HS)
        for C in (1, 3, 4):
            for mode in ("bilinear", "threshold"):
                for N in (1, 3):
                    imgs = _images(N, C, mode, seed=10 * C + N)
                    want, want_valid = undistort_numpy(imgs, cam, out_cam, mode)
                    for want_plane in (True, False):
                        got, valid = _device(imgs, cam, out_cam, mode, want_valid=want_plane)
                        assert got.shape == (N, Hd, Wd, C)
                        assert np.array_equal(got, want), (model, C, mode, N)
                        if want_plane:
                            assert np.array_equal(valid, want_valid), (model, C, mode, N)
        n_invalid += int((~want_valid).sum())
        n_valid += int(want_valid.sum())
    assert n_valid > 0 and (n_invalid > 0 or Wd * Hd == 1)


@pytest.mark.parametrize("model", UC.MODELS)
def test_principal_point_far_outside(model):
    """A whole side of the output is invalid (and, with the source's principal point off the image, most of it)."""
    from utils.undistort import undistort_numpy
    imgs = UC.noise(3, HS, WS, 3, seed=3)
    for cam, out_cam in ((UC.camera(model, WS, HS), UC.pinhole(66, 13, 36.0, 36.0, cx=-20.0, cy=30.0)),
                         (UC.camera(model, WS, HS, c=(-30.0, 50.0)), UC.pinhole(37, 11, 30.0, 30.0))):
        want, want_valid = undistort_numpy(imgs, cam, out_cam, "bilinear")
        got, valid = _device(imgs, cam, out_cam, "bilinear")
        assert np.array_equal(valid, want_valid) and np.array_equal(got, want)
        assert (~want_valid).sum() > want_valid.size // 3
        assert np.all(got[:, ~valid] == 0)


@pytest.mark.parametrize("model", UC.MODELS)
def test_kernel_equals_numpy_path_at_640x480(model):
    from utils.undistort import undistort_numpy, undistorted_camera
    cam = UC.camera(model, 640, 480)
    out_cam = undistorted_camera(cam, blank_pixels=0.5)
    imgs = UC.noise(1, 480, 640, 3, seed=7)
    want, want_valid = undistort_numpy(imgs, cam, out_cam, "bilinear")
    got, valid = _device(imgs, cam, out_cam, "bilinear")
    assert (~want_valid).any() and want_valid.sum() > 200000
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(got, want)


def test_pinhole_source_is_copied():
    from data.colmap import Camera
    cam = Camera(1, "PINHOLE", WS, HS, np.array([40.0, 41.0, 22.5, 15.5]))
    imgs = UC.noise(2, HS, WS, 4)
    got, valid = _device(imgs, cam, cam, "bilinear")
    assert valid.all() and np.array_equal(got, imgs)


def test_repeatable_and_stream_independent():
    from utils.undistort import undistort_device, undistorted_camera
    cam = UC.camera("FULL_OPENCV", 131, 77)
    out_cam = undistorted_camera(cam, blank_pixels=1.0)
    src = torch.from_numpy(UC.noise(3, 77, 131, 3, seed=2)).cuda()
    a, va = undistort_device(src, cam, out_cam, "bilinear")
    b, vb = undistort_device(src, cam, out_cam, "bilinear")
    assert torch.equal(a, b) and torch.equal(va, vb)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c, vc = undistort_device(src, cam, out_cam, "bilinear")
    side.synchronize()
    assert torch.equal(a, c) and torch.equal(va, vc)


def test_device_path_refuses_a_host_tensor():
    import hgs_runtime as rt
    from utils.undistort import undistort_device
    cam = UC.camera("RADIAL", WS, HS)
    with pytest.raises(rt.HgsError):
        undistort_device(torch.from_numpy(UC.noise(1, HS, WS, 3)), cam, UC.pinhole(8, 8, 10.0, 10.0), "bilinear")


def test_driver_writes_the_same_files_on_both_devices(tmp_path):
    """PNG inputs only: no encoder stands between the two paths' bytes."""
    import undistort
    from tests.test_undistort_cpu import check_driver_scene
    src, out_gpu, out_cpu = str(tmp_path / "src"), str(tmp_path / "gpu"), str(tmp_path / "cpu")
    cams, images = UC.build_scene(src)
    assert undistort.main(["-s", src, "-o", out_gpu, "--device", "cuda", "--batch", "2"]) == 3
    assert undistort.main(["-s", src, "-o", out_cpu, "--device", "cpu"]) == 3
    a, b = UC.tree_bytes(out_gpu), UC.tree_bytes(out_cpu)
    assert sorted(a) == sorted(b) and len(a) == 3 + 3 + 1
    for name in a:
        assert a[name] == b[name], name
    check_driver_scene(src, out_gpu, cams, images)
    assert os.path.exists(os.path.join(out_gpu, "masks", "view_1.png"))
