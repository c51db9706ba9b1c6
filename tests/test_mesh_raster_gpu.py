"""The rasterizer of the dataset synthesis on the GPU (csrc/hgs_raster.hip through scene/mesh_renderer.py): images, masks and gray
views equal to the CPU path's bit for bit (which also needs the device's float64 sqrt and division to round correctly); dropped
counts; errors before any launch; synthesize.py on the device against the CPU; and a synthesized scene feeding training and
evaluation."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image as PILImage

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _scene(n_strands=300, n_seg=40, seed=0, model=np.eye(4), hair_lit=True, head=True):
    import synthetic
    from scene.mesh_renderer import Lighting, MeshModel
    from tests.synth_fixtures import sphere_mesh
    walks = synthetic.strand_polylines(n_strands, n_seg, seed=seed)
    S, K, _ = walks.shape
    verts = walks.reshape(-1, 3)
    base = np.arange(S)[:, None] * K + np.arange(K - 1)[None]
    edges = np.stack([base, base + 1], -1).reshape(-1, 2)
    rng = np.random.default_rng(seed)
    cols = np.repeat(rng.uniform(0.2, 1, (S, 4)), K, 0)
    nrm = rng.normal(size=verts.shape)
    models = []
    if head:
        v, f, n = sphere_mesh(0.08, 20, 40)
        models.append(MeshModel(v, faces=f, colors=np.array([0.0, 0, 0, 1]), normals=n, use_lighting=False))
        models.append(MeshModel(v, faces=f, colors=np.array([0.75, 0.75, 0.75, 1]), normals=n, model=model, ka=0.5, kd=0.5))
    models.append(MeshModel(verts, edges=edges, colors=cols, normals=nrm, use_lighting=hair_lit, model=model))
    light = Lighting(light_pos=np.array([0, 5, 5]), ambient_color=np.ones(4), diffuse_color=np.ones(4))
    return models, light


def _cams(n, W, H, seed=0):
    from synthesize import camera_matrices
    from utils.camera import generate_cameras
    pose = np.eye(4)
    pose[:3, 3] = [0, -0.05, 0.45]
    pose[:3, 1:3] *= -1
    cams, Es = generate_cameras(max(n, 2), H, W, cam_pose=pose, anchor_pos=np.array([0, -0.05, 0]), offset=0.45,
                                focal_length_px=0.9 * max(W, H))
    ids, views, projs = camera_matrices(cams, Es)
    return views[:n], projs[:n]


def _same(models, light, views, projs, W, H, mesh_indices=None, label=""):
    from scene.mesh_renderer import render_views
    img_c, drop_c, gray_c = render_views(models, views, projs, W, H, light, mesh_indices=mesh_indices, return_gray=True)
    img_g, drop_g, gray_g = render_views(models, views, projs, W, H, light, mesh_indices=mesh_indices, return_gray=True,
                                         device="cuda")
    img_g, gray_g = img_g.cpu().numpy(), gray_g.cpu().numpy()
    assert img_g.shape == img_c.shape and drop_g == drop_c
    diff = (img_g != img_c).any(axis=-1)
    assert not diff.any(), f"{label}: {int(diff.sum())} pixel(s) differ"
    assert np.array_equal(gray_g, gray_c)
    return img_c, drop_c


@pytest.mark.parametrize("W,H", [(160, 120), (17, 33), (1000, 1000)])
@pytest.mark.parametrize("width", [1.0, 2.0, 3.5])
def test_device_equals_cpu(W, H, width):
    models, light = _scene(n_strands=400 if W > 200 else 150)
    models[-1].line_width = width
    views, projs = _cams(5 if W < 1000 else 2, W, H)
    img, _ = _same(models, light, views, projs, W, H, mesh_indices=[1, 2], label=f"{W}x{H} w={width}")
    assert (img != 0).any()
    _same(models, light, views, projs, W, H, mesh_indices=[0, 2])
    _same(models, light, views[:1], projs[:1], W, H)


def test_unlit_and_model_matrix():
    a = np.deg2rad(20)
    M = np.array([[np.cos(a), 0, np.sin(a), 0.01], [0, 1.2, 0, -0.02], [-np.sin(a), 0, np.cos(a), 0.0], [0, 0, 0, 1]])
    for lit in (True, False):
        models, light = _scene(n_strands=200, model=M, hair_lit=lit)
        views, projs = _cams(5, 160, 120)
        _same(models, light, views, projs, 160, 120, label=f"lit={lit}")


def test_odd_primitive_count_and_hot_tile():
    from scene.mesh_renderer import MeshModel
    models, light = _scene(n_strands=7, n_seg=9, head=False)           # 63 segments: not a multiple of 64
    assert models[0].indices.shape[0] % 64 != 0
    views, projs = _cams(3, 160, 120)
    _same(models, light, views, projs, 160, 120)
    # > 10^4 short segments crossing one 32x32 tile
    rng = np.random.default_rng(5)
    c = np.array([0.0, -0.05, 0.0])
    p = c + rng.normal(scale=0.002, size=(12000, 3))
    q = p + rng.normal(scale=0.002, size=(12000, 3))
    verts = np.concatenate([p, q])
    edges = np.stack([np.arange(12000), np.arange(12000) + 12000], 1)
    hot = MeshModel(verts, edges=edges, colors=np.repeat(rng.uniform(0.1, 1, (12000, 4)), 2, 0), normals=rng.normal(size=verts.shape))
    _same([hot], light, views, projs, 160, 120, label="hot tile")


def test_drops_and_errors():
    from scene.mesh_renderer import MeshModel, render_views
    views, projs = _cams(2, 64, 48)
    v = np.array([[0, -0.05, 0], [0.01, -0.05, 0], [0, -0.05, 3.0], [0.01, -0.04, 0], [0, -0.05, -8], [0.02, -0.05, 0]])
    m = MeshModel(v, edges=np.array([[0, 1], [2, 3], [4, 5]]))
    t = MeshModel(v, faces=np.array([[0, 1, 3], [2, 1, 3]]))
    _, dc = render_views([m, t], views, projs, 64, 48)
    _, dg = render_views([m, t], views, projs, 64, 48, device="cuda")
    assert dc == dg and dc > 0
    with pytest.raises(ValueError):
        render_views([], views, projs, 64, 48, device="cuda")
    with pytest.raises(IndexError):
        render_views([m], views, projs, 64, 48, mesh_indices=[0, 3], device="cuda")


def test_opengl_renderer_names_on_the_device():
    from scene.OpenGLRenderer import OpenGLCamera, OpenGLLighting, OpenGLModel, OpenGLRenderer
    models, light = _scene(n_strands=100)
    views, projs = _cams(2, 96, 64)
    out = {}
    for dev in (None, "cuda"):
        r = OpenGLRenderer(resolution=(96, 64), device=dev)
        r.lighting = OpenGLLighting(light_pos=np.array([0, 5, 5]), ambient_color=np.ones(4), diffuse_color=np.ones(4))
        for m in models:
            r.models.append(OpenGLModel(m.vertices, edges=m.indices if m.kind == 2 else None, faces=m.indices if m.kind == 3 else None,
                                        colors=m.colors, normals=m.normals, use_lighting=m.use_lighting))
        r.setup()
        r.camera = OpenGLCamera(views[1], projs[1])
        r.setup_camera()
        img = r.render(mesh_indices=[1, 2])
        out[dev] = img if dev is None else img.cpu().numpy()
    assert np.array_equal(out[None], out["cuda"]) and out[None].shape == (64, 96, 3)


def _synth(tmp_path, device, W=128, H=96, cams=4, extra=()):
    import synthesize
    from tests.synth_fixtures import sphere_mesh, write_obj, write_usc
    hair, head = tmp_path / "strands.data", tmp_path / "head.obj"
    if not hair.exists():
        write_usc(str(hair), n_long=200, seed=2)
        v, f, n = sphere_mesh()
        write_obj(str(head), v, f, n)
    out = tmp_path / f"scene_{device}"
    synthesize.main(["--dataset", "usc_hair_salon", "--hair", str(hair), "--head", str(head), "-o", str(out), "--pct_strands", "2",
                     "--cameras", str(cams), "--height", str(H), "--width", str(W), "--cam_z", "0.45", "--device", device, *extra])
    return out


def test_synthesize_cuda_equals_cpu(tmp_path):
    from utils.vision import _cpu_responses, gabor_kernels, to_gray
    cpu, gpu = _synth(tmp_path, "cpu"), _synth(tmp_path, "cuda", extra=("--batch", "3"))
    for sub in ("images", "masks"):
        names = sorted(os.listdir(cpu / sub))
        assert names == sorted(os.listdir(gpu / sub)) and len(names) == 4
        for n in names:
            assert (cpu / sub / n).read_bytes() == (gpu / sub / n).read_bytes(), (sub, n)
    for n in ("sparse/0/cameras.bin", "sparse/0/images.bin", "sparse/0/points3D.bin", "hair_eval_data.npz",
              "head_reconstruction_data.npz"):
        assert (cpu / n).read_bytes() == (gpu / n).read_bytes(), n
    # orientation maps: equal except where a response lies within 1e-6 of a half-integer (tests/test_orientation_gpu.py)
    _, kernels = gabor_kernels()
    total = excluded = 0
    for n in sorted(os.listdir(cpu / "images")):
        gray = to_gray(np.asarray(PILImage.open(cpu / "images" / n)))
        _, near = _cpu_responses(gray, kernels, near=1e-6)
        stem = n.split(".")[0]
        for k in ("orientation", "confidence"):
            a = np.asarray(PILImage.open(cpu / "orientations" / f"{stem}_{k}.png"))
            b = np.asarray(PILImage.open(gpu / "orientations" / f"{stem}_{k}.png"))
            assert np.array_equal(a[~near], b[~near]), (n, k)
        total += near.size
        excluded += int(near.sum())
    print(f"orientation maps: {excluded} of {total} pixel(s) excluded")
    assert excluded <= 1e-3 * total


def test_synthesized_scene_trains_and_evaluates(tmp_path):
    from arguments import OptimizationParams
    from scene import Scene
    from train import training_step
    src = _synth(tmp_path, "cuda", W=160, H=120, cams=6, extra=("--use_gt_hair_verts",))
    model = tmp_path / "model"
    args = SimpleNamespace(source_path=str(src), model_path=str(model), images="images", sh_degree=0, resolution=-1,
                           data_device="cuda", eval=False)
    scene = Scene(args, shuffle=False)
    cams = scene.getCameras()
    assert len(cams) == 6 and all(c.mask is not None and c.orientation_field is not None for c in cams)
    opt = OptimizationParams()
    opt.enable_topology = False
    scene.gaussians.training_setup(opt)
    bg = torch.zeros(3, device="cuda")
    losses = []
    for it in range(1, 301):
        loss, _, _ = training_step(scene.gaussians, cams[it % len(cams)], opt, bg, it, extent=scene.cameras_extent)
        losses.append(float(loss))
    first, last = np.mean(losses[:20]), np.mean(losses[-20:])
    print(f"stage I loss {first:.4f} -> {last:.4f}")
    assert np.isfinite(losses).all() and last < first
    scene.save(300)
    metrics = tmp_path / "metrics.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "hair-gs_amd", "eval.py"), "-s", str(src), "-p", str(model), "--device",
                        "cuda", "--json", str(metrics)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout[-800:])
    import json
    m = json.loads(metrics.read_text())
    assert m and all(np.isfinite(v) for v in _numbers(m))


def _numbers(d):
    for v in d.values():
        if isinstance(v, dict):
            yield from _numbers(v)
        elif isinstance(v, (int, float)):
            yield float(v)
