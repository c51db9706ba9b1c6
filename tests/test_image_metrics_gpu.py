"""Image metrics on the GPU (hair-gs_amd/csrc/hgs_view_stats.hip through loss/image_metrics.py, and view_metrics.py): the kernel
against the CPU path on random planes for every combination of absent planes (the within counts may differ only by the
pixels the float64 reference calls ambiguous), bitwise reproducibility and batch independence,
and the driver end to end on a trained Stage-I cloud and on the strand model merge.py makes from it."""
import itertools
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = ("mask_count", "fg_count", "inter_count", "orient_count")
SSE = ("sse", "sse_hair")
ORIENT = ("orient_abs_sum", "orient_weighted_sum")


def _planes(V, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    fg = r(V, H, W)
    fg[:, ::3, ::2] = 0.5                            # exactly at the threshold
    mask = r(V, H, W) > 0.4
    omap = r(V, 3, H, W) * 2 - 1
    omap[:, :, ::4, :] = 0.0                         # pixels nothing was blended into
    if V > 1:                                         # a view with empty masks
        mask[1] = False
        fg[1] = 0.0
    q = torch.linalg.qr(torch.randn(V, 3, 3, generator=g)).Q
    vm = torch.eye(4).repeat(V, 1, 1)
    vm[:, :3, :3] = q
    vm[:, 3, :3] = torch.randn(V, 3, generator=g)
    return dict(pred_rgb=r(V, 3, H, W) * 1.4 - 0.2, gt_rgb=r(V, 3, H, W), fg=fg, gt_mask=mask, omap=omap, viewmats=vm,
                gt_theta=r(V, H, W) * math.pi, confidence=r(V, H, W))


def _subset(p, fg, mask, omap, conf):
    kw = dict(pred_rgb=p["pred_rgb"], gt_rgb=p["gt_rgb"])
    if fg:
        kw["fg"] = p["fg"]
    if mask:
        kw["gt_mask"] = p["gt_mask"]
    if omap:
        kw.update(omap=p["omap"], viewmats=p["viewmats"], gt_theta=p["gt_theta"])
    if conf:
        kw["confidence"] = p["confidence"]
    return kw


def _ambiguous(p, with_mask):
    """Per view, the number of orientation pixels within the float64 reference's margin of the 10 and of the 20 degree edge
    (tests/view_stats_reference.py): only there may two float32 evaluations count differently."""
    from loss.image_metrics import MIN_VAL
    from tests import view_stats_reference as VR
    res = []
    for v in range(p["omap"].shape[0]):
        omap = p["omap"][v].numpy()
        om = p["gt_mask"][v].numpy() if with_mask else (omap != 0).any(axis=0)
        res.append(VR.ambiguous_counts(omap, p["viewmats"][v].numpy(), MIN_VAL, p["gt_theta"][v].numpy(), om))
    return res


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("V,H,W", [(3, 7, 5), (3, 96, 64), (1, 1080, 1920)])
def test_kernel_matches_the_cpu_path(V, H, W):
    from loss.image_metrics import view_metrics
    p = _planes(V, H, W, seed=H)
    allowed = {mask: _ambiguous(p, mask) for mask in (False, True)}
    worst = 0
    for fg, mask, omap, conf in itertools.product((False, True), repeat=4):
        kw = _subset(p, fg, mask, omap, conf)
        cpu = view_metrics(**kw)
        gpu = view_metrics(**{k: v.cuda() for k, v in kw.items()})
        for v, (c, g) in enumerate(zip(cpu, gpu)):
            assert {k for k, v in c.items() if v is None} == {k for k, v in g.items() if v is None}
            for k in COUNTS:
                assert c[k] == g[k], (k, fg, mask, omap, conf)
            for k in SSE:
                if c[k] is not None:
                    assert c[k] == g[k] or _rel(g[k], c[k]) <= 1e-10, (k, c[k], g[k])
            for k in ORIENT:
                if c[k] is not None:
                    assert c[k] == g[k] or _rel(g[k], c[k]) <= 1e-5, (k, c[k], g[k])
            if c["orient_count"] is not None:
                for k, amb in zip(("orient_within_10_count", "orient_within_20_count"), allowed[mask][v]):
                    d = abs(c[k] - g[k])
                    worst = max(worst, d)
                    assert d <= amb, (k, c[k], g[k], amb)
            assert abs(c["ssim"] - g["ssim"]) <= 2e-5 and abs(c["l1"] - g["l1"]) <= 2e-5
            assert c["psnr"] == g["psnr"] or abs(c["psnr"] - g["psnr"]) <= 1e-9
    print(f"V={V} {H}x{W}: largest within-count difference {worst}")


def test_bitwise_reproducible_and_independent_of_the_batch():
    from loss.image_metrics import view_metrics
    for H, W in ((96, 64), (1080, 1920)):
        p = {k: v.cuda() for k, v in _planes(4, H, W, seed=7).items()}
        a = view_metrics(**p)
        b = view_metrics(**p)
        assert a == b
        for v in range(4):
            alone = view_metrics(**{k: t[v:v + 1] for k, t in p.items()})[0]
            assert alone == a[v], (H, W, v)


def _check_driver(src, model, tmp_path, tag):
    import view_metrics as cli
    from loss.image_metrics import METRICS, render_planes, view_metrics
    from scene import Scene
    j1, j2 = tmp_path / f"{tag}1.json", tmp_path / f"{tag}2.json"
    res = cli.main(["-s", str(src), "-m", str(model), "--batch", "3", "--per_view", "--json", str(j1), "--quiet"])
    cli.main(["-s", str(src), "-m", str(model), "--json", str(j2), "--quiet"])
    assert j1.read_bytes() == j2.read_bytes()                        # (--batch 3 and the default 8 alike)
    back = json.loads(j1.read_text())
    assert list(back["views"]) == [f"v{i:02d}" for i in range(4)] == list(res["views"])
    for name, m in res["views"].items():
        for k in ("psnr", "ssim", "l1", "psnr_hair", "mask_iou", "orient_err_deg", "orient_within_10", "orient_loss"):
            assert m[k] is not None and math.isfinite(m[k]), (name, k)
    for k in METRICS:
        vals = [v[k] for v in res["views"].values()]
        assert res["mean"][k] == math.fsum(vals) / len(vals)
    # the per-view numbers are view_metrics' on renders made here, one view at a time
    scene = Scene(cli.parse_args(["-s", str(src), "-m", str(model)]), shuffle=False)
    for cam in scene.getCameras():
        rgb, fg, omap = render_planes(cam, scene.gaussians)
        m = view_metrics(rgb[None], cam.original_image[None], fg=fg[None], gt_mask=cam.mask[None], omap=omap[None],
                         viewmats=cam.world_view_transform[None], gt_theta=cam.orientation_field[None],
                         confidence=cam.orientation_confidence[None], min_val=scene.gaussians.min_val)[0]
        assert {k: m[k] for k in METRICS} == res["views"][cam.image_name], cam.image_name
    return res, scene


def test_driver_on_a_trained_cloud_and_its_strand_model(tmp_path):
    from tests.test_dataset_io_cpu import _write_capture, _write_side_files
    import merge as merge_cli
    import train as train_cli
    from scene.gaussian_model import GaussianModel
    from scene.hair_gaussian_model import HairGaussianModel
    src, model = tmp_path / "capture", tmp_path / "out"
    _write_capture(src, n_views=4, W=96, H=64)
    _write_side_files(src)
    train_cli.main(["-s", str(src), "-m", str(model), "--iterations", "30", "--save_frequency", "30", "--quiet",
                    "--densify_from_iter", "5", "--densification_interval", "10", "--densify_grad_threshold", "1e-7"])
    res, scene = _check_driver(src, model, tmp_path, "cloud")
    assert isinstance(scene.gaussians, GaussianModel) and res["iteration"] == 30
    merge_cli.main(["-s", str(src), "-m", str(model), "--iterations", "5"])
    res2, scene2 = _check_driver(src, model, tmp_path, "strands")
    assert isinstance(scene2.gaussians, HairGaussianModel) and res2["iteration"] > 30
    assert os.path.exists(tmp_path / "strands1.json")
