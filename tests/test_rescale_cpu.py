"""Rescaling without a GPU (hair-gs_amd/utils/rescale.py, hair-gs_amd/rescale.py): the numpy path against the term-by-term restatement
of tests/rescale_reference.py, the properties of the double-angle pair rule, its agreement with the closed form, the camera and
keypoint rule, the C entry points' refusals, and the driver's scene read back by the loader."""
import os

import numpy as np
import pytest

from tests import rescale_cases as RC
from tests import rescale_reference as REF

# (source W x H, output W' x H'): one pixel, an integer factor to one pixel, fractional factors with a remainder on both axes, integer
# factors 2 and 3, the identity, and everything into one pixel
SIZES = [((1, 1), (1, 1)), ((2, 2), (1, 1)), ((5, 3), (2, 1)), ((7, 5), (3, 2)), ((8, 8), (4, 4)), ((9, 9), (3, 3)),
         ((45, 31), (45, 31)), ((45, 31), (1, 1))]
_ID = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SIZES]


@pytest.mark.parametrize("src,dst", SIZES, ids=_ID)
def test_numpy_images_equal_the_loop_restatement(src, dst):
    from utils.rescale import rescale_images
    (W, H) = src
    for C in (1, 3, 4):
        for mode in ("average", "threshold"):
            imgs = RC.noise(2, H, W, C, seed=C) if mode == "average" else np.repeat(RC.binary_masks(2, H, W, seed=C), C, axis=3)
            got = rescale_images(imgs, dst, mode)
            assert got.dtype == np.uint8 and got.shape == (2, dst[1], dst[0], C)
            assert np.array_equal(got, REF.rescale(imgs, dst, mode)), (C, mode)
            if src == dst and mode == "average":
                assert np.array_equal(got, imgs)


@pytest.mark.parametrize("src,dst", SIZES, ids=_ID)
def test_numpy_pairs_equal_the_loop_restatement(src, dst):
    from utils.rescale import rescale_orientation
    (W, H) = src
    tabs = REF.tables()
    for planes in (RC.pair_planes(2, H, W, seed=3), RC.smooth_pair_planes(2, H, W, seed=4)):
        t, c, m = planes
        for mask in (m, None):
            got_t, got_c = rescale_orientation(t, c, mask, dst)
            want_t, want_c = REF.rescale_orientation(t, c, mask, dst, tabs)
            assert got_t.dtype == got_c.dtype == np.uint8 and got_t.shape == got_c.shape == (2, dst[1], dst[0])
            assert np.array_equal(got_t, want_t) and np.array_equal(got_c, want_c)
            assert got_t.max() < 255


def test_tables_are_the_restatements():
    from utils.rescale import orientation_tables
    tab = orientation_tables()
    for k, want in enumerate(REF.tables()):
        assert np.array_equal(tab[k], np.array(want))
    assert tab[0, 255] == tab[0, 0] == 1.0 and tab[1, 255] == tab[1, 0] == 0.0


@pytest.mark.parametrize("src,dst", [(4, 2), (3, 1), (5, 2)], ids=["factor2", "factor3", "5to2"])
def test_uniform_box_comes_back(src, dst):
    """A plane of one repeated pair (t, c) gives (t mod 255, c) everywhere: every t, c in {1, 17, 200, 255}."""
    from utils.rescale import rescale_orientation
    ts, cs = np.meshgrid(np.arange(256), np.array([1, 17, 200, 255]), indexing="ij")
    ts, cs = ts.reshape(-1).astype(np.uint8), cs.reshape(-1).astype(np.uint8)
    t = np.broadcast_to(ts[:, None, None], (ts.size, src, src)).copy()
    c = np.broadcast_to(cs[:, None, None], (ts.size, src, src)).copy()
    got_t, got_c = rescale_orientation(t, c, None, (dst, dst))
    assert np.array_equal(got_t, np.broadcast_to((ts % 255)[:, None, None], got_t.shape))
    assert np.array_equal(got_c, np.broadcast_to(cs[:, None, None], got_c.shape))


def _one_box(t, c, m=None):
    from utils.rescale import rescale_orientation
    a = lambda v: None if v is None else np.array(v, np.uint8).reshape(1, 2, 2)   # noqa: E731
    got_t, got_c = rescale_orientation(a(t), a(c), a(m), (1, 1))
    want = REF.rescale_orientation(a(t), a(c), a(m), (1, 1))
    assert (got_t[0, 0, 0], got_c[0, 0, 0]) == (want[0][0, 0, 0], want[1][0, 0, 0])
    return int(got_t[0, 0, 0]), int(got_c[0, 0, 0])


def test_pair_rule_at_the_wrap_and_on_disagreement():
    assert _one_box([1, 254, 254, 1], [255] * 4) == (0, 255)           # the two sides of the 0 / 255 wrap: a linear mean would say 127
    t, c = _one_box([0, 128, 128, 0], [255] * 4)                        # perpendicular directions cancel
    print(f"bytes 0 and 128 in equal parts: confidence byte {c}")
    assert c <= 3
    assert _one_box([10, 200, 77, 31], [0] * 4) == (0, 0)              # no confidence anywhere
    assert _one_box([10, 200, 77, 31], [255] * 4, [0] * 4) == (0, 0)   # wholly outside the mask
    assert _one_box([10, 200, 77, 31], [90, 255, 255, 255], [255, 0, 0, 0]) == (10, 90)   # the mask gates: one pixel counts


def test_angle_byte_agrees_with_the_closed_form():
    """3000 random 2 x 2 boxes: the boundary count against floor(((atan2(Y, X) mod 2 pi)/2)*255/pi + 0.5) mod 255.  The closed form rounds
    atan2 and four more operations, so a box within that rounding of a boundary may come out one code away: at most 1 % of them
    (measured: none)."""
    from utils.rescale import orientation_tables, rescale_orientation
    rng = np.random.default_rng(0)
    t = rng.integers(0, 256, (3000, 2, 2), dtype=np.uint8)
    c = rng.integers(1, 256, (3000, 2, 2), dtype=np.uint8)
    got, _ = rescale_orientation(t, c, None, (1, 1))
    tab = orientation_tables()
    X, Y = (c * tab[0][t]).sum(axis=(1, 2)), (c * tab[1][t]).sum(axis=(1, 2))
    want = (np.floor(((np.arctan2(Y, X) % (2 * np.pi)) / 2) * 255 / np.pi + 0.5) % 255).astype(np.int64)
    diff = (got[:, 0, 0].astype(np.int64) - want) % 255
    n_diff = int((diff != 0).sum())
    print(f"{n_diff} of 3000 boxes differ from the closed form")
    assert n_diff <= 30
    assert np.all((diff == 0) | (diff == 1) | (diff == 254))


def test_rescaled_camera_and_keypoints():
    from data.colmap import Camera
    from utils.rescale import rescale_keypoints, rescaled_camera
    cam = Camera(7, "PINHOLE", 3208, 2200, np.array([2500.0, 2510.0, 1600.5, 1099.25]))
    out = rescaled_camera(cam, (1604, 1100))
    assert (out.id, out.model, out.width, out.height) == (7, "PINHOLE", 1604, 1100)
    assert np.array_equal(out.params, [2500.0 * 1604 / 3208, 2510.0 * 1100 / 2200, 1600.5 * 1604 / 3208, 1099.25 * 1100 / 2200])
    out = rescaled_camera(cam, (1600, 1097))                                    # (the -1 rule: int(2200 / (3208 / 1600)))
    assert np.array_equal(out.params, [2500.0 * 1600 / 3208, 2510.0 * 1097 / 2200, 1600.5 * 1600 / 3208, 1099.25 * 1097 / 2200])
    simple = Camera(2, "SIMPLE_PINHOLE", 48, 36, np.array([40.0, 24.5, 17.5]))
    out = rescaled_camera(simple, (24, 18))                                     # equal ratios: it stays SIMPLE_PINHOLE
    assert out.model == "SIMPLE_PINHOLE" and np.array_equal(out.params, [20.0, 12.25, 8.75])
    out = rescaled_camera(simple, (23, 18))                                     # unequal ratios: PINHOLE
    assert (out.model, out.width, out.height) == ("PINHOLE", 23, 18)
    assert np.array_equal(out.params, [40.0 * 23 / 48, 40.0 * 18 / 36, 24.5 * 23 / 48, 17.5 * 18 / 36])
    xys = np.array([[0.0, 0.0], [48.0, 36.0], [10.5, 20.25]])
    assert np.array_equal(rescale_keypoints(xys, simple, out), np.column_stack([xys[:, 0] * 23 / 48, xys[:, 1] * 18 / 36]))
    assert rescale_keypoints(np.zeros((0, 2)), simple, out).shape == (0, 2)
    with pytest.raises(ValueError, match="enlarging"):
        rescaled_camera(simple, (49, 36))


@pytest.mark.parametrize("model", ["SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV", "OPENCV_FISHEYE"])
def test_distorted_models_are_refused_by_name(model):
    from data.colmap import CAMERA_MODEL_NAMES, Camera
    from utils.rescale import rescaled_camera
    cam = Camera(1, model, 32, 24, np.full(CAMERA_MODEL_NAMES[model].num_params, 0.01))
    with pytest.raises(ValueError, match=f"{model} .*run undistort.py first"):
        rescaled_camera(cam, (16, 12))


def test_bad_arguments_are_refused():
    from utils.rescale import rescale_images, rescale_orientation
    imgs = RC.noise(1, 24, 32, 3)
    with pytest.raises(ValueError, match="mode"):
        rescale_images(imgs, (16, 12), "nearest")
    with pytest.raises(ValueError, match="shape"):
        rescale_images(RC.noise(1, 24, 32, 2), (16, 12))
    with pytest.raises(ValueError, match="enlarging"):
        rescale_images(imgs, (33, 12))
    with pytest.raises(ValueError, match="enlarging"):
        rescale_images(imgs, (16, 25))
    with pytest.raises(ValueError, match="0 x 12"):
        rescale_images(imgs, (0, 12))
    with pytest.raises(ValueError, match="device"):
        rescale_images(imgs, (16, 12), device="cpu")
    t, c, m = RC.pair_planes(1, 24, 32)
    with pytest.raises(ValueError, match="confidence"):
        rescale_orientation(t, c[:, :12], None, (16, 12))
    with pytest.raises(ValueError, match="enlarging"):
        rescale_orientation(t, c, m, (64, 12))
    with pytest.raises(ValueError, match="device"):
        rescale_orientation(t, c, m, (16, 12), device="cpu")


def test_abi_holds_the_new_entry_points_at_version_15():
    import hgs_runtime as rt
    assert "hgs_rescale_images" in rt.SIGNATURES and "hgs_rescale_orientation" in rt.SIGNATURES
    assert rt.ABI_VERSION == 15 and rt.lib().hgs_abi_version() == 15


def test_abi_refuses_bad_arguments():
    """The C entry points check their arguments before they touch a pointer or launch anything (no GPU needed)."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    buf = (C.c_ubyte * 16)()
    b = C.addressof(buf)
    for N, Cn, Hs, Ws, Hd, Wd, mode, words in ((0, 3, 8, 8, 4, 4, 0, b"sizes"), (1, 3, 8, 0, 4, 4, 0, b"sizes"), (1, 3, 8, 8, 0, 4, 0, b"sizes"),
                                               (1, 2, 8, 8, 4, 4, 0, b"channels"), (1, 3, 8, 8, 4, 4, 2, b"mode"),
                                               (1, 3, 8, 8, 9, 4, 0, b"enlarging"), (1, 3, 8, 8, 4, 9, 0, b"enlarging"),
                                               (1, 4, 40000, 40000, 4, 4, 0, b"2^31"), (70000, 1, 8, 8, 4, 4, 0, b"grid"),
                                               (1, 1, 70000, 8, 66000, 4, 0, b"grid")):
        assert L.hgs_rescale_images(None, N, Cn, Hs, Ws, Hd, Wd, b, b, mode) != 0
        assert words in L.hgs_last_error(), words
    assert L.hgs_rescale_images(None, 1, 3, 8, 8, 4, 4, None, b, 0) != 0 and b"null" in L.hgs_last_error()
    assert L.hgs_rescale_images(None, 1, 3, 8, 8, 4, 4, b, None, 0) != 0 and b"null" in L.hgs_last_error()
    for N, Hs, Ws, Hd, Wd, words in ((0, 8, 8, 4, 4, b"sizes"), (1, 8, 8, 4, 9, b"enlarging"), (1, 50000, 50000, 4, 4, b"2^31"),
                                     (70000, 8, 8, 4, 4, b"grid")):
        assert L.hgs_rescale_orientation(None, N, Hs, Ws, Hd, Wd, b, b, None, b, b, b) != 0
        assert words in L.hgs_last_error(), words
    for k in (0, 1, 3, 4, 5):                        # (the mask alone may be NULL)
        args = [b] * 6
        args[k] = None
        assert L.hgs_rescale_orientation(None, 1, 8, 8, 4, 4, *args) != 0 and b"null" in L.hgs_last_error()


def check_driver_scene(src, out, cams, images, resolution=2, pairs=("view_1", "view_2")):
    """What the driver must have written under `out` for the scene of RC.build_scene under `src` (shared with the GPU test)."""
    from data.colmap import read_extrinsics_binary, read_intrinsics_binary
    from data.dataset_readers import readColmapSceneInfo
    from scene.scene import target_size
    from utils.rescale import rescale_keypoints, rescaled_camera
    new_cams = read_intrinsics_binary(os.path.join(out, "sparse", "0", "cameras.bin"))
    assert set(new_cams) == set(cams)
    for cid, cam in cams.items():
        want = rescaled_camera(cam, target_size(cam.width, cam.height, resolution))
        assert (new_cams[cid].model, new_cams[cid].width, new_cams[cid].height) == (want.model, want.width, want.height)
        assert np.array_equal(new_cams[cid].params, want.params)
    assert new_cams[1].model == "PINHOLE" and new_cams[2].model == ("PINHOLE" if resolution == 2 else "SIMPLE_PINHOLE")
    new_images = read_extrinsics_binary(os.path.join(out, "sparse", "0", "images.bin"))
    assert set(new_images) == set(images)
    for k, im in images.items():
        got = new_images[k]
        assert got.name == im.name and got.camera_id == im.camera_id
        assert np.array_equal(got.qvec, im.qvec) and np.array_equal(got.tvec, im.tvec) and np.array_equal(got.point3D_ids, im.point3D_ids)
        assert np.array_equal(got.xys, rescale_keypoints(im.xys, cams[im.camera_id], new_cams[im.camera_id]))
    with open(os.path.join(src, "sparse", "0", "points3D.bin"), "rb") as a, open(os.path.join(out, "sparse", "0", "points3D.bin"), "rb") as b:
        assert a.read() == b.read()
    for name in RC.SIDE_FILES:
        with open(os.path.join(src, name), "rb") as a, open(os.path.join(out, name), "rb") as b:
            assert a.read() == b.read()
    before = {c.image_name: c for c in readColmapSceneInfo(src).cameras}
    info = readColmapSceneInfo(out)
    assert len(info.cameras) == 4
    for c in info.cameras:
        s = before[c.image_name]
        assert c.image.size == (c.width, c.height) == target_size(s.width, s.height, resolution)
        assert abs(c.FovX - s.FovX) <= 1e-12 * s.FovX and abs(c.FovY - s.FovY) <= 1e-12 * s.FovY
        assert (c.mask is None) == (s.mask is None) and c.image.mode == s.image.mode and c.image.format == s.image.format
        if c.mask is not None:
            assert c.mask.shape == (c.height, c.width) and c.mask.any() and not c.mask.all()
        if c.image_name in pairs:
            assert c.orientation_field.shape == c.orientation_confidence.shape == (c.height, c.width)
            assert c.orientation_confidence.max() > 0.3
        else:
            assert c.orientation_field is None and c.orientation_confidence is None
    assert {c.image.mode for c in info.cameras} == {"RGB", "RGBA"} and {c.image.format for c in info.cameras} == {"PNG", "JPEG"}


def test_driver_cpu(tmp_path, capsys):
    import rescale
    from PIL import Image as PILImage
    from utils.rescale import rescale_images, rescale_orientation
    src, out = str(tmp_path / "src"), str(tmp_path / "out")
    cams, images = RC.build_scene(src)
    assert rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", "2", "--batch", "2"]) == 4
    said = capsys.readouterr().out
    assert "4 image(s), 2 mask(s) and 2 orientation pair(s)" in said and "48 x 36 -> 24 x 18" in said and "45 x 31 -> 22 x 16" in said
    check_driver_scene(src, out, cams, images)
    # the files hold what the module computes from the source files: view_1's image, mask and pair (gated by the source mask)
    load = lambda *p: np.asarray(PILImage.open(os.path.join(*p)))   # noqa: E731
    assert np.array_equal(load(out, "images", "view_1.png"), rescale_images(load(src, "images", "view_1.png")[None], (24, 18))[0])
    mask = load(src, "masks", "view_1.png")
    assert np.array_equal(load(out, "masks", "view_1.png"), rescale_images(mask[None, :, :, None], (24, 18), "threshold")[0, :, :, 0])
    t, c = rescale_orientation(load(src, "orientations", "view_1_orientation.png")[None], load(src, "orientations", "view_1_confidence.png")[None],
                               mask[None], (24, 18))
    assert np.array_equal(load(out, "orientations", "view_1_orientation.png"), t[0])
    assert np.array_equal(load(out, "orientations", "view_1_confidence.png"), c[0])
    assert c[0][0, 0] == 0 and c[0].max() > 100            # (outside the mask; inside it)
    with pytest.raises(SystemExit, match="not empty"):
        rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", "2"])
    before = RC.tree_bytes(out)
    assert rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", "2", "--overwrite"]) == 4
    after = RC.tree_bytes(out)
    assert os.path.join("sparse", "0", "points3D.ply") in before and os.path.join("sparse", "0", "points3D.ply") not in after   # stale: removed
    before.pop(os.path.join("sparse", "0", "points3D.ply"))
    assert before == after


def test_driver_refusals(tmp_path):
    import rescale
    from data.colmap import read_intrinsics_binary, write_cameras_binary
    src, out = str(tmp_path / "src"), str(tmp_path / "out")
    RC.build_scene(src)
    for r in ("1", "-1"):                                         # (-1: no image is wider than 1600)
        with pytest.raises(SystemExit, match="nothing to do"):
            rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", r])
    with pytest.raises(SystemExit, match="enlarging"):
        rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", "47"])      # (a target width between the two cameras' widths)
    with pytest.raises(SystemExit, match="must not be the source"):
        rescale.main(["-s", src, "-o", os.path.join(src, "."), "--device", "cpu", "-r", "2"])
    with pytest.raises(SystemExit, match="cuda or cpu"):
        rescale.main(["-s", src, "-o", out, "--device", "tpu", "-r", "2"])
    assert not os.path.exists(out)
    os.remove(os.path.join(src, "orientations", "view_2_confidence.png"))
    with pytest.raises(SystemExit, match="only one of"):
        rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", "2"])
    assert not os.path.exists(out)
    cams_path = os.path.join(src, "sparse", "0", "cameras.bin")
    cams = read_intrinsics_binary(cams_path)
    cams[2] = cams[2]._replace(model="SIMPLE_RADIAL", params=np.array([38.0, 22.1, 15.2, -0.1]))
    write_cameras_binary(cams, cams_path)
    with pytest.raises(SystemExit, match="SIMPLE_RADIAL .*run undistort.py first"):
        rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", "2", "--orientations", "skip"])


def test_driver_orientation_modes_and_target_width(tmp_path, capsys):
    import shutil
    import rescale
    from data.dataset_readers import readColmapSceneInfo
    src = str(tmp_path / "src")
    cams, images = RC.build_scene(src)
    skip, est, wide = str(tmp_path / "skip"), str(tmp_path / "est"), str(tmp_path / "wide")
    assert rescale.main(["-s", src, "-o", skip, "--device", "cpu", "-r", "2", "--orientations", "skip"]) == 4
    assert "orient.py must be run" in capsys.readouterr().out and not os.path.exists(os.path.join(skip, "orientations"))
    assert rescale.main(["-s", src, "-o", est, "--device", "cpu", "-r", "2", "--orientations", "estimate"]) == 4
    assert "must be run" not in capsys.readouterr().out
    for c in readColmapSceneInfo(est).cameras:                  # orient.py ran on the result: every view has its maps
        assert c.orientation_field.shape == c.orientation_confidence.shape == (c.height, c.width)
    # a target width: camera 1 (48 x 36) comes out 24 x 18, camera 2 (45 x 31, down by 1.875) 24 x 16
    assert rescale.main(["-s", src, "-o", wide, "--device", "cpu", "-r", "24"]) == 4
    sizes = {c.image_name: c.image.size for c in readColmapSceneInfo(wide).cameras}
    assert sizes == {"view_1": (24, 18), "view_2": (24, 18), "view_3": (24, 16), "view_4": (24, 16)}
    # a scene without orientations/: nothing is averaged by default, and asking for it is refused
    shutil.rmtree(os.path.join(src, "orientations"))
    bare = str(tmp_path / "bare")
    with pytest.raises(SystemExit, match="does not exist"):
        rescale.main(["-s", src, "-o", bare, "--device", "cpu", "-r", "2", "--orientations", "average"])
    assert rescale.main(["-s", src, "-o", bare, "--device", "cpu", "-r", "2"]) == 4
    assert "0 orientation pair(s)" in capsys.readouterr().out and not os.path.exists(os.path.join(bare, "orientations"))


def test_driver_reads_a_text_model(tmp_path):
    import rescale
    src, out_b, out_t = str(tmp_path / "src"), str(tmp_path / "out_b"), str(tmp_path / "out_t")
    cams, images = RC.build_scene(src)
    rescale.main(["-s", src, "-o", out_b, "--device", "cpu", "-r", "2"])
    sparse = os.path.join(src, "sparse", "0")
    with open(os.path.join(sparse, "cameras.txt"), "w") as fh:
        for c in cams.values():
            fh.write(f"{c.id} {c.model} {c.width} {c.height} " + " ".join(repr(float(v)) for v in c.params) + "\n")
    with open(os.path.join(sparse, "images.txt"), "w") as fh:
        for im in images.values():
            fh.write(f"{im.id} " + " ".join(repr(float(v)) for v in list(im.qvec) + list(im.tvec)) + f" {im.camera_id} {im.name}\n")
            fh.write(" ".join(f"{float(x)!r} {float(y)!r} {int(p)}" for (x, y), p in zip(im.xys, im.point3D_ids)) + "\n")
    with open(os.path.join(sparse, "points3D.txt"), "w") as fh:
        fh.write("1 0.0 0.5 1.0 10 20 30 0.25 1 0\n")
    for f in ("cameras.bin", "images.bin", "points3D.bin"):
        os.remove(os.path.join(sparse, f))
    rescale.main(["-s", src, "-o", out_t, "--device", "cpu", "-r", "2"])
    a, b = RC.tree_bytes(out_b), RC.tree_bytes(out_t)
    assert b.pop(os.path.join("sparse", "0", "points3D.txt")) == b"1 0.0 0.5 1.0 10 20 30 0.25 1 0\n"
    a.pop(os.path.join("sparse", "0", "points3D.bin"))
    assert a == b
