"""Image metrics without a GPU (hair-gs_amd/loss/image_metrics.py, hair-gs_amd/view_metrics.py): hand-built views with known
answers (PSNR of a constant offset, identical images, mask IoU, the orientation wrap-around, the 10 / 20 degree edges, every
combination of absent planes), the CPU path against the training loss's own statements (_orientation_term, losses.ssim), and the
driver's argument parsing and JSON."""
import itertools
import json
import math
import types

import numpy as np
import pytest
import torch


def _planes(V=2, H=6, W=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    omap = r(V, 3, H, W) * 2 - 1
    omap[:, :, 0, :] = 0.0                           # (rows nothing was blended into)
    q = torch.linalg.qr(torch.randn(V, 3, 3, generator=g)).Q
    vm = torch.eye(4).repeat(V, 1, 1)
    vm[:, :3, :3] = q
    return dict(pred_rgb=r(V, 3, H, W) * 1.4 - 0.2, gt_rgb=r(V, 3, H, W), fg=r(V, H, W), gt_mask=r(V, H, W) > 0.5, omap=omap,
                viewmats=vm, gt_theta=r(V, H, W) * math.pi, confidence=r(V, H, W))


def test_constant_offset_is_20_db_and_equal_images_are_inf():
    from loss.image_metrics import view_metrics
    gt = torch.full((1, 3, 8, 6), 0.25)
    m = view_metrics(gt + 0.1, gt, gt_mask=torch.ones(1, 8, 6, dtype=torch.bool))[0]
    assert abs(m["psnr"] - 20.0) < 1e-5 and abs(m["psnr_hair"] - 20.0) < 1e-5
    assert abs(m["l1"] - 0.1) < 1e-6 and m["pixels"] == 48
    m = view_metrics(gt.clone(), gt, gt_mask=torch.ones(1, 8, 6, dtype=torch.bool))[0]
    assert m["psnr"] == math.inf and m["psnr_hair"] == math.inf and m["l1"] == 0.0 and m["sse"] == 0.0
    # an empty GT mask: no hair PSNR
    m = view_metrics(gt + 0.1, gt, gt_mask=torch.zeros(1, 8, 6, dtype=torch.bool))[0]
    assert m["psnr_hair"] is None and m["mask_count"] == 0.0
    # the render is clamped to [0, 1] before it is compared
    assert view_metrics(gt * 0 + 1.5, gt * 0 + 1.0)[0]["psnr"] == math.inf


def test_psnr_hair_counts_only_the_mask():
    from loss.image_metrics import view_metrics
    gt = torch.zeros(1, 3, 4, 4)
    pred = gt.clone()
    pred[0, :, 0, 0] = 0.5                            # an error outside the mask only
    mask = torch.zeros(1, 4, 4, dtype=torch.bool)
    mask[0, 2:, :] = True
    m = view_metrics(pred, gt, gt_mask=mask)[0]
    assert m["psnr_hair"] == math.inf and m["mask_count"] == 8.0
    assert abs(m["psnr"] - 10 * math.log10(48 / 0.75)) < 1e-9


def test_mask_iou_of_known_masks():
    from loss.image_metrics import view_metrics
    gt = torch.zeros(2, 3, 4, 4)
    mask = torch.zeros(2, 4, 4, dtype=torch.bool)
    mask[0, :, :2] = True                             # left half: 8 pixels
    fg = torch.zeros(2, 4, 4)
    fg[0, :2, :] = 0.5                                # top half at exactly the threshold: foreground
    fg[0, 2:, :] = float(np.nextafter(np.float32(0.5), np.float32(0)))   # just below: not
    m0, m1 = view_metrics(gt, gt, fg=fg, gt_mask=mask)
    assert m0["inter_count"] == 4.0 and m0["union_count"] == 12.0 and m0["mask_iou"] == pytest.approx(1 / 3, abs=0)
    assert m0["fg_count"] == 8.0
    assert m1["mask_iou"] == 1.0 and m1["union_count"] == 0.0      # both empty
    assert view_metrics(gt, gt, fg=fg)[0]["mask_iou"] is None      # no GT mask


def _theta_zero_omap(H, W):
    """A direction image whose angle is exactly 0 at every pixel under the identity view: pix = (0, 1)."""
    omap = torch.zeros(1, 3, H, W)
    omap[0, 1] = 1.0
    return omap


def test_orientation_wraps_around():
    from loss.image_metrics import view_metrics
    a = math.radians(-1.0)                            # atan2(sin a, cos a) = -1 deg -> 179 deg
    omap = torch.zeros(1, 3, 2, 2)
    omap[0, 0], omap[0, 1] = math.sin(a), math.cos(a)
    m = view_metrics(torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, 2), omap=omap, viewmats=torch.eye(4)[None],
                     gt_theta=torch.full((1, 2, 2), math.radians(1.0)))[0]
    assert abs(m["orient_err_deg"] - 2.0) < 1e-4 and m["orient_count"] == 4.0
    assert m["orient_within_10"] == 1.0 and m["orient_loss"] == pytest.approx(math.radians(2.0), rel=1e-5)


def _edge_pair(th):
    """(g_in, g_out): float32 GT angles whose difference from theta = 0 is the largest <= th and the smallest > th, the
    difference evaluated as the contract does in float32."""
    hp = np.float32(np.pi / 2)
    g = np.float32(th)
    for _ in range(8):
        g = np.nextafter(g, np.float32(0))
    cands = []
    for _ in range(32):
        d = hp - np.abs(np.abs(np.float32(0) - g) - hp)
        cands.append((g, d))
        g = np.nextafter(g, np.float32(1))
    g_in = max((c for c in cands if c[1] <= th), key=lambda c: c[1])
    g_out = min((c for c in cands if c[1] > th), key=lambda c: c[1])
    return g_in, g_out


@pytest.mark.parametrize("deg", [10, 20])
def test_within_counts_at_the_exact_edges(deg):
    from loss.image_metrics import TH10, TH20, view_metrics
    th = TH10 if deg == 10 else TH20
    (g_in, d_in), (g_out, d_out) = _edge_pair(th)
    assert d_in <= th < d_out
    gt_theta = torch.tensor([[[float(g_in), float(g_out)], [float(g_in), 0.0]]])
    z = torch.zeros(1, 3, 2, 2)
    m = view_metrics(z, z, omap=_theta_zero_omap(2, 2), viewmats=torch.eye(4)[None], gt_theta=gt_theta)[0]
    assert m[f"orient_within_{deg}_count"] == 3.0 and m["orient_count"] == 4.0
    print(f"{deg} deg edge: in {float(d_in)!r} out {float(d_out)!r} threshold {float(th)!r}")


def test_absent_planes_give_none():
    from loss.image_metrics import METRICS, view_metrics
    p = _planes()
    ori = ("orient_err_deg", "orient_within_10", "orient_within_20", "orient_loss")
    for fg, mask, omap, conf in itertools.product((False, True), repeat=4):
        kw = dict(pred_rgb=p["pred_rgb"], gt_rgb=p["gt_rgb"])
        if fg:
            kw["fg"] = p["fg"]
        if mask:
            kw["gt_mask"] = p["gt_mask"]
        if omap:
            kw.update(omap=p["omap"], viewmats=p["viewmats"], gt_theta=p["gt_theta"])
        if conf:
            kw["confidence"] = p["confidence"]
        for m in view_metrics(**kw):
            assert set(METRICS) <= set(m)
            assert m["psnr"] is not None and m["ssim"] is not None and m["l1"] is not None
            assert (m["psnr_hair"] is None) == (not mask)
            assert (m["mask_iou"] is None) == (not (mask and fg))
            for k in ori:
                assert (m[k] is None) == (not omap), (k, fg, mask, omap, conf)
            if omap and not conf:
                assert m["orient_loss"] == m["orient_abs_sum"] / m["orient_count"]     # weight 1
    # the orientation statistics are off when the GT angle is absent, and a map without view matrices is refused
    assert view_metrics(p["pred_rgb"], p["gt_rgb"], omap=p["omap"], viewmats=p["viewmats"])[0]["orient_loss"] is None
    with pytest.raises(ValueError):
        view_metrics(p["pred_rgb"], p["gt_rgb"], omap=p["omap"], gt_theta=p["gt_theta"])
    with pytest.raises(ValueError):
        view_metrics(p["pred_rgb"], p["gt_rgb"][:, :, :-1])


@pytest.mark.parametrize("with_mask", [True, False])
def test_orient_loss_is_the_training_term(monkeypatch, with_mask):
    import loss.losses as L
    from loss.image_metrics import view_metrics
    monkeypatch.setattr(L, "fused_losses", False)
    p = _planes(V=3, H=17, W=13, seed=4)
    out = view_metrics(p["pred_rgb"], p["gt_rgb"], gt_mask=p["gt_mask"] if with_mask else None, omap=p["omap"],
                       viewmats=p["viewmats"], gt_theta=p["gt_theta"], confidence=p["confidence"])
    for v, m in enumerate(out):
        cam = types.SimpleNamespace(world_view_transform=p["viewmats"][v], orientation_field=p["gt_theta"][v],
                                    orientation_confidence=p["confidence"][v], mask=p["gt_mask"][v] if with_mask else None)
        ref = float(L._orientation_term(p["omap"][v], types.SimpleNamespace(min_val=1e-7), cam, torch.zeros(3)))
        assert m["orient_loss"] == pytest.approx(ref, rel=1e-6, abs=0)
        n = int(p["gt_mask"][v].sum()) if with_mask else int((p["omap"][v] != 0).any(0).sum())
        assert m["orient_count"] == n


def test_ssim_and_l1_are_the_loss_functions_on_the_clamped_render():
    import loss.losses as L
    from loss.image_metrics import view_metrics
    p = _planes(V=2, H=23, W=19, seed=2)
    for v, m in enumerate(view_metrics(p["pred_rgb"], p["gt_rgb"])):
        pred = p["pred_rgb"][v].clamp(0, 1)
        assert m["ssim"] == float(L.ssim(pred, p["gt_rgb"][v]))
        assert m["l1"] == float(L.l1_loss(pred, p["gt_rgb"][v]))


def test_cpu_path_against_float64_sums():
    """The sums of the CPU path against a plain numpy evaluation (float32 per pixel, float64 sums)."""
    from loss.image_metrics import view_metrics
    p = _planes(V=2, H=9, W=7, seed=5)
    out = view_metrics(p["pred_rgb"], p["gt_rgb"], fg=p["fg"], gt_mask=p["gt_mask"])
    pred = np.clip(p["pred_rgb"].numpy(), 0, 1)
    e = (pred - p["gt_rgb"].numpy()) ** 2
    mk = p["gt_mask"].numpy()
    for v, m in enumerate(out):
        assert m["sse"] == pytest.approx(e[v].astype(np.float64).sum(), rel=1e-12)
        assert m["sse_hair"] == pytest.approx(e[v][:, mk[v]].astype(np.float64).sum(), rel=1e-12)
        P = p["fg"].numpy()[v] >= 0.5
        assert m["inter_count"] == (P & mk[v]).sum() and m["union_count"] == (P | mk[v]).sum()


def test_driver_arguments_and_json(tmp_path):
    import view_metrics as cli
    a = cli.parse_args(["-s", str(tmp_path / "cap"), "-m", str(tmp_path / "model"), "--batch", "3", "--per_view", "--json",
                        str(tmp_path / "o.json")])
    assert a.batch == 3 and a.per_view and a.json.endswith("o.json") and a.source_path.endswith("cap")
    d = cli.parse_args(["-s", "x", "-m", str(tmp_path / "model")])
    assert d.batch == 8 and not d.per_view and d.json is None
    with pytest.raises(SystemExit):
        cli.parse_args(["-s", "x", "-m", str(tmp_path / "model"), "--batch", "0"])
    from loss.image_metrics import METRICS
    base = {k: 0.5 for k in METRICS}
    per_view = {"b.png": dict(base, psnr=30.0, mask_iou=None), "a.png": dict(base, psnr=math.inf, mask_iou=0.25, extra=1)}
    res = cli.summarize("m", 30, per_view)
    assert list(res["views"]) == ["a.png", "b.png"] and set(res["views"]["a.png"]) == set(METRICS)
    assert res["mean"]["mask_iou"] == 0.25 and res["mean"]["psnr"] == math.inf and res["mean"]["ssim"] == 0.5
    text = cli.to_json(res)
    back = json.loads(text)
    assert set(back) == {"model", "iteration", "views", "mean"} and back["iteration"] == 30
    assert back["views"]["a.png"]["psnr"] is None and back["views"]["b.png"]["mask_iou"] is None
    assert back["mean"]["psnr"] is None and back["views"]["b.png"]["psnr"] == 30.0
    assert "NaN" not in text and "Infinity" not in text
    table = cli.format_table(res, per_view=True)
    assert "a.png" in table and "psnr_hair" in table
    with pytest.raises(SystemExit):
        cli.main(["-s", str(tmp_path / "cap"), "-m", str(tmp_path / "model")])     # no trained model there
