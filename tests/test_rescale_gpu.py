"""hgs_rescale_images and hgs_rescale_orientation (csrc/hgs_rescale.hip) against the numpy path of utils/rescale.py: the bytes are
equal, at the smallest shapes where the kernels can go wrong -- output widths around the 64-lane wavefront and past one 256-lane
workgroup, one row and odd row counts, integer and fractional factors on either axis, one and three planes, 1 / 3 / 4 channels on rows
of odd byte length, both modes, the mask given and NULL -- and on one 640 x 480 -> 320 x 240 case per entry point."""
import numpy as np
import pytest
import torch

from tests import rescale_cases as RC

pytestmark = pytest.mark.gpu

# (source W x H, output W' x H'): the output widths 1, 3, 63, 64, 65, 257 and heights 1 and odd counts; 130 -> 65, 9 -> 3, 771 -> 257 and
# 10 -> 5 are integer factors, 129 -> 64, 45 -> 7, 131 -> 63, 31 -> 5 and the others fractional; 45 x 31 -> 45 x 31 is the identity
SHAPES = [((45, 31), (1, 1)), ((9, 9), (3, 3)), ((45, 31), (3, 5)), ((45, 31), (7, 1)), ((131, 10), (63, 5)), ((129, 7), (64, 3)),
          ((130, 9), (65, 9)), ((771, 4), (257, 3)), ((300, 5), (257, 1)), ((45, 31), (45, 31))]
_ID = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES]


def _device_images(images, size, mode):
    from utils.rescale import rescale_device
    return rescale_device(torch.from_numpy(images).cuda(), size, mode).cpu().numpy()


def _device_pairs(t, c, m, size):
    from utils.rescale import rescale_orientation_device
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()   # noqa: E731
    out_t, out_c = rescale_orientation_device(dev(t), dev(c), dev(m), size)
    return out_t.cpu().numpy(), out_c.cpu().numpy()


@pytest.mark.parametrize("src,dst", SHAPES, ids=_ID)
def test_image_kernel_equals_numpy_path(src, dst):
    """C x mode x N in {1, 3} (three different planes)."""
    from utils.rescale import rescale_numpy
    (W, H) = src
    for C in (1, 3, 4):
        for mode in ("average", "threshold"):
            for N in (1, 3):
                imgs = RC.noise(N, H, W, C, seed=10 * C + N) if mode == "average" else \
                    np.ascontiguousarray(np.repeat(RC.binary_masks(N, H, W, seed=10 * C + N), C, axis=3))
                got = _device_images(imgs, dst, mode)
                assert got.shape == (N, dst[1], dst[0], C)
                assert np.array_equal(got, rescale_numpy(imgs, dst, mode)), (C, mode, N)


@pytest.mark.parametrize("src,dst", SHAPES, ids=_ID)
def test_orientation_kernel_equals_numpy_path(src, dst):
    """Noise and coherent planes x N in {1, 3} x mask given / NULL."""
    from utils.rescale import rescale_orientation_numpy
    (W, H) = src
    for make in (RC.pair_planes, RC.smooth_pair_planes):
        for N in (1, 3):
            t, c, m = make(N, H, W, seed=N)
            for mask in (m, None):
                want_t, want_c = rescale_orientation_numpy(t, c, mask, dst)
                got_t, got_c = _device_pairs(t, c, mask, dst)
                assert got_t.shape == got_c.shape == (N, dst[1], dst[0])
                assert np.array_equal(got_t, want_t), (make.__name__, N, mask is None)
                assert np.array_equal(got_c, want_c), (make.__name__, N, mask is None)


def test_uniform_boxes_come_back_from_the_kernel():
    """Every (t, c in {1, 17, 200, 255}) as a uniform 5 x 5 plane -> 2 x 2: (t mod 255, c), the property the nearest-code rule is for."""
    ts, cs = np.meshgrid(np.arange(256), np.array([1, 17, 200, 255]), indexing="ij")
    ts, cs = ts.reshape(-1).astype(np.uint8), cs.reshape(-1).astype(np.uint8)
    t = np.broadcast_to(ts[:, None, None], (ts.size, 5, 5)).copy()
    c = np.broadcast_to(cs[:, None, None], (ts.size, 5, 5)).copy()
    got_t, got_c = _device_pairs(t, c, None, (2, 2))
    assert np.array_equal(got_t, np.broadcast_to((ts % 255)[:, None, None], got_t.shape))
    assert np.array_equal(got_c, np.broadcast_to(cs[:, None, None], got_c.shape))


def test_kernels_equal_numpy_path_at_640x480():
    from utils.rescale import rescale_numpy, rescale_orientation_numpy
    imgs = RC.noise(1, 480, 640, 3, seed=7)
    assert np.array_equal(_device_images(imgs, (320, 240), "average"), rescale_numpy(imgs, (320, 240), "average"))
    t, c, m = RC.smooth_pair_planes(1, 480, 640, seed=8)
    want_t, want_c = rescale_orientation_numpy(t, c, m, (320, 240))
    got_t, got_c = _device_pairs(t, c, m, (320, 240))
    assert want_c.max() > 200 and (want_c == 0).any()
    assert np.array_equal(got_t, want_t) and np.array_equal(got_c, want_c)


def test_repeatable_and_stream_independent():
    from utils.rescale import rescale_device, rescale_orientation_device
    src = torch.from_numpy(RC.noise(3, 77, 131, 3, seed=2)).cuda()
    t, c, m = (torch.from_numpy(a).cuda() for a in RC.pair_planes(3, 77, 131, seed=2))
    a, pa = rescale_device(src, (50, 31), "average"), rescale_orientation_device(t, c, m, (50, 31))
    b, pb = rescale_device(src, (50, 31), "average"), rescale_orientation_device(t, c, m, (50, 31))
    assert torch.equal(a, b) and torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d, pd = rescale_device(src, (50, 31), "average"), rescale_orientation_device(t, c, m, (50, 31))
    side.synchronize()
    assert torch.equal(a, d) and torch.equal(pa[0], pd[0]) and torch.equal(pa[1], pd[1])


def test_device_path_refuses_a_host_tensor_and_enlarging():
    import hgs_runtime as rt
    from utils.rescale import rescale_device, rescale_orientation_device
    with pytest.raises(rt.HgsError):
        rescale_device(torch.from_numpy(RC.noise(1, 31, 45, 3)), (8, 8), "average")
    t, c, m = (torch.from_numpy(a) for a in RC.pair_planes(1, 31, 45))
    with pytest.raises(rt.HgsError):
        rescale_orientation_device(t.cuda(), c, None, (8, 8))
    with pytest.raises(ValueError, match="enlarging"):
        rescale_device(torch.from_numpy(RC.noise(1, 31, 45, 3)).cuda(), (46, 31), "average")


def test_driver_writes_the_same_files_on_both_devices(tmp_path):
    import rescale
    from tests.test_rescale_cpu import check_driver_scene
    src, out_gpu, out_cpu = str(tmp_path / "src"), str(tmp_path / "gpu"), str(tmp_path / "cpu")
    cams, images = RC.build_scene(src)
    assert rescale.main(["-s", src, "-o", out_gpu, "--device", "cuda", "-r", "2", "--batch", "2"]) == 4
    assert rescale.main(["-s", src, "-o", out_cpu, "--device", "cpu", "-r", "2"]) == 4
    a, b = RC.decoded(out_gpu), RC.decoded(out_cpu)
    assert sorted(a) == sorted(b) and len(a) == 4 + 2 + 4
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    a, b = RC.tree_bytes(out_gpu), RC.tree_bytes(out_cpu)
    assert sorted(a) == sorted(b) and len(a) == 10 + 3 + 3
    for name in a:                                   # (the same bytes went into the same encoders)
        assert a[name] == b[name], name
    check_driver_scene(src, out_gpu, cams, images)
