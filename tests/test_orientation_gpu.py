"""Orientation maps on the GPU (csrc/hgs_vision.hip through utils/vision.py): the same uint8 responses, field and confidence as
the CPU path, bit for bit, except at pixels where some CPU pre-rounding response lies within 1e-6 of a half-integer (there the two
summation orders may round apart); batching; limits and errors; orient.py on the device; and its maps feeding a training step."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image as PILImage

pytestmark = pytest.mark.gpu

EPS = 1e-6
# Pixels excluded at most.  At the default 180 angles about 90 responses per pixel fall inside [-0.5, 255.5], each within 1e-6 of a
# half-integer with probability 2e-6: about 2e-4 of the pixels of noise or a render sit on a boundary.
MAX_EXCLUDED = 1e-3


def _cpu(gray, ks, A):
    from utils.vision import _confidence, _cpu_responses, _field_variance, gabor_kernels
    thetas, kernels = gabor_kernels(ks, num_angles=A)
    stack, near = _cpu_responses(gray, kernels, near=EPS)
    idx, var = _field_variance(stack, thetas)
    return thetas[idx], _confidence(var), stack, near


def _compare(gray, ks=31, A=180, label=""):
    from utils.vision import estimate_orientation_fields
    field_c, conf_c, stack, near = _cpu(gray, ks, A)
    f, c, r = estimate_orientation_fields(torch.from_numpy(gray)[None].cuda(), ks, num_angles=A, return_responses=True)
    f, c, r = f[0].cpu().numpy(), c[0].cpu().numpy(), r[0].cpu().numpy()
    n_ex = int(near.sum())
    print(f"{label} {gray.shape} ks={ks} A={A}: {n_ex} of {near.size} pixel(s) excluded")
    assert n_ex <= MAX_EXCLUDED * near.size, n_ex
    assert f.dtype == np.float64 and c.dtype == np.float32 and r.shape == gray.shape + (A,)
    keep = ~near
    assert np.array_equal(r[keep], stack.transpose(1, 2, 0)[keep])
    assert np.array_equal(f[keep], field_c[keep])
    assert np.array_equal(c[keep], conf_c[keep])
    return n_ex


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _render(W, H, n_strands, seed=0):
    """Gray uint8 view of a synthetic strand model's RGB render."""
    from synthetic import build_capture
    from utils.vision import to_gray
    _, _, cams, _ = build_capture((n_strands, False, 1, W, H), seed=seed)
    img = (cams[0].original_image.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
    return to_gray(img)


@pytest.mark.parametrize("ks,A", [(31, 180), (7, 180), (8, 180), (31, 16), (7, 16), (8, 16)])
@pytest.mark.parametrize("shape", [(48, 64), (17, 33), (5, 7)])
def test_noise_equals_cpu(shape, ks, A):
    _compare(_noise(shape, 11), ks, A, "noise")


@pytest.mark.parametrize("phi", [0, 30, 60, 100, 150])
def test_gratings_equal_cpu(phi):
    y, x = np.mgrid[0:96, 0:80]
    p = np.deg2rad(phi)
    img = np.clip(np.rint(127.5 + 60 * np.cos(2 * np.pi * (x * np.cos(p) + y * np.sin(p)) / 8)), 0, 255).astype(np.uint8)
    for ks, A in ((31, 180), (8, 16)):
        _compare(img, ks, A, f"grating {phi}")


def test_strand_render_256_equals_cpu():
    gray = _render(256, 256, 300)
    assert gray.std() > 1
    for ks, A in ((31, 180), (7, 16)):
        _compare(gray, ks, A, "render")


def test_strand_render_1000_equals_cpu():
    _compare(_render(1000, 1000, 1000, seed=1), 31, 180, "render")


def test_batch_equals_single_calls():
    from utils.vision import estimate_orientation_fields
    views = np.stack([_noise((40, 56), s) for s in range(3)])
    f, c, r = estimate_orientation_fields(torch.from_numpy(views).cuda(), return_responses=True)
    for i in range(3):
        fi, ci, ri = estimate_orientation_fields(torch.from_numpy(views[i:i + 1]).cuda(), return_responses=True)
        assert torch.equal(f[i], fi[0]) and torch.equal(c[i], ci[0]) and torch.equal(r[i], ri[0])


def test_device_limits_and_errors():
    from utils.vision import NoVarianceError, estimate_orientation_field, estimate_orientation_fields
    g = torch.from_numpy(_noise((2, 16, 16), 0))
    for kw in (dict(num_angles=1), dict(num_angles=257), dict(kernel_size=64), dict(kernel_size=0)):
        with pytest.raises(ValueError):
            estimate_orientation_fields(g, **kw)          # a host tensor: the limits are checked before anything touches the GPU
        with pytest.raises(ValueError):
            estimate_orientation_field(g[0].numpy(), device="cuda", **kw)
    estimate_orientation_fields(g.cuda(), kernel_size=63, num_angles=256)
    estimate_orientation_fields(g.cuda(), kernel_size=62, num_angles=3)   # (2 angles: theta = pi repeats 0, no variance)
    with pytest.raises(ValueError):
        estimate_orientation_field(np.zeros((16, 16), np.uint8), device="cuda")
    views = torch.from_numpy(np.stack([_noise((16, 16), 1), np.zeros((16, 16), np.uint8), _noise((16, 16), 2)])).cuda()
    with pytest.raises(NoVarianceError) as e:
        estimate_orientation_fields(views)
    assert e.value.views == [1]
    with pytest.raises(TypeError):
        estimate_orientation_fields(views.float())


def _views(seed, n, shape):
    return {f"v{i:02d}.png": np.random.default_rng(seed + i).integers(0, 256, shape + (3,), dtype=np.uint8) for i in range(n)}


def test_orient_cli_cuda_writes_the_cpu_files(tmp_path):
    import orient
    from utils.vision import to_gray
    views = _views(50, 3, (40, 48))
    for _, v in views.items():
        assert not _cpu(to_gray(v), 31, 180)[3].any()     # (no pixel on a rounding boundary: the files must be byte-identical)
    for d in ("cpu", "cuda"):
        (tmp_path / d / "images").mkdir(parents=True)
        for name, v in views.items():
            PILImage.fromarray(v).save(tmp_path / d / "images" / name)
        assert orient.main(["-s", str(tmp_path / d), "--device", d, "--batch", "2"]) == 3
    names = sorted(os.listdir(tmp_path / "cpu" / "orientations"))
    assert names == sorted(os.listdir(tmp_path / "cuda" / "orientations")) and len(names) == 6
    for n in names:
        assert (tmp_path / "cpu" / "orientations" / n).read_bytes() == (tmp_path / "cuda" / "orientations" / n).read_bytes(), n


def test_orient_maps_load_and_train(tmp_path):
    """A COLMAP capture without orientations/ -> orient.py on the GPU -> Scene -> training steps with the orientation term."""
    from tests.test_dataset_io_cpu import _write_capture
    import orient
    from arguments import OptimizationParams
    from scene import Scene
    from train import training_step
    src, model = tmp_path / "capture", tmp_path / "out"
    _write_capture(src, n_views=3, W=64, H=48)
    shutil.rmtree(src / "orientations")
    assert orient.main(["-s", str(src), "--device", "cuda"]) == 3
    args = SimpleNamespace(source_path=str(src), model_path=str(model), images="images", sh_degree=0, resolution=-1,
                           data_device="cuda", eval=False)
    scene = Scene(args, shuffle=False)
    cams = scene.getCameras()
    assert len(cams) == 3
    for cam in cams:
        o = np.asarray(PILImage.open(src / "orientations" / f"{cam.image_name}_orientation.png"))
        c = np.asarray(PILImage.open(src / "orientations" / f"{cam.image_name}_confidence.png"))
        assert cam.orientation_field is not None and cam.orientation_confidence is not None
        assert torch.equal(cam.orientation_field.cpu(), torch.from_numpy(o.astype(np.float32) * np.pi / 255.0))
        assert torch.equal(cam.orientation_confidence.cpu(), torch.from_numpy(c.astype(np.float32) / 255.0))
        assert c.max() == 255
    opt = OptimizationParams()
    opt.enable_topology = False
    scene.gaussians.training_setup(opt)
    bg = torch.zeros(3, device="cuda")
    for it in range(1, 4):
        loss, _, _ = training_step(scene.gaussians, cams[it % 3], opt, bg, it, extent=scene.cameras_extent)
        assert torch.isfinite(loss)
