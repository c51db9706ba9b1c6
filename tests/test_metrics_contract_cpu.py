"""The match predicate the GPU strand metrics implement (csrc/hgs_metrics.hip, loss/metrics.py oriented_match) against scipy's
cKDTree on points placed on the distance boundary, and eval.py's CPU path end to end."""
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RADIUS = 4e-3


def boundary_fixture(radius=RADIUS, n_disagree=1000, seed=0):
    """Pairs (a_i, b_i), 0.1 apart from every other pair, whose distance lies within a few ulps of `radius`, holding at least
    n_disagree pairs where d2 = (dx*dx + dy*dy) + dz*dz <= r*r and sqrt(d2) <= r disagree.  Returns (a, b, d2 <= r*r)."""
    rng = np.random.default_rng(seed)
    keep_a, keep_b, flips, start, n = [], [], 0, 0, 20000
    while flips < n_disagree:
        cell = np.stack(np.unravel_index(np.arange(start, start + n), (64, 64, 64)), 1)
        start += n
        b = cell * 0.1 + 1.0 + rng.uniform(0.0, 0.01, (n, 3))
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        a = b + radius * u
        a[:, 0] -= 128 * np.spacing(a[:, 0])
        hit, flip = a.copy(), np.zeros(n, bool)
        for _ in range(256):                                   # walk x across the boundary one ulp at a time
            d = a - b
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            new = ((d2 <= radius * radius) != (np.sqrt(d2) <= radius)) & ~flip
            hit[new], flip = a[new], flip | new
            a[:, 0] = np.nextafter(a[:, 0], np.inf)
        a = np.where(flip[:, None], hit, b + radius * u)
        pick = flip | (rng.uniform(size=n) < 0.05)
        keep_a.append(a[pick]); keep_b.append(b[pick])
        flips += int(flip.sum())
    a, b = np.concatenate(keep_a), np.concatenate(keep_b)
    d = a - b
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return a, b, d2 <= radius * radius


def test_boundary_fixture_has_disagreeing_pairs():
    a, b, inside = boundary_fixture()
    d = a - b
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert int(((d2 <= RADIUS * RADIUS) != (np.sqrt(d2) <= RADIUS)).sum()) >= 1000
    assert 0 < inside.sum() < len(inside)


def test_documented_predicate_equals_ckdtree_on_the_boundary():
    """d2 = (dx*dx + dy*dy) + dz*dz <= r*r, float64 in that order, is the form cKDTree.query_ball_point decides by."""
    from scipy.spatial import cKDTree
    a, b, inside = boundary_fixture()
    lists = cKDTree(b).query_ball_point(a, r=RADIUS)
    found = np.array([len(x) > 0 for x in lists])
    assert all(set(x) <= {i} for i, x in enumerate(lists))     # (each point's only candidate is its partner)
    assert np.array_equal(found, inside)


def _strand_capture(root, seed=0, n_strands=40, n_seg=20, noise=1e-3):
    """A capture's hair_eval_data.npz from synthetic strands and a strand model of the same strands moved by ~noise."""
    import torch
    from synthetic import strand_polylines
    from scene.hair_gaussian_model import HairGaussianModel
    from scene.ply_io import save_hair_ply
    pts = strand_polylines(n_strands, n_seg, seed=seed).astype(np.float64)
    os.makedirs(root, exist_ok=True)
    np.savez(os.path.join(root, "hair_eval_data.npz"), points=pts[:, :-1].reshape(-1, 3),
             directions=(pts[:, 1:] - pts[:, :-1]).reshape(-1, 3), points_id_to_strand_id=np.repeat(np.arange(n_strands), n_seg))
    moved = (pts + np.random.default_rng(seed + 1).normal(size=pts.shape) * noise).astype(np.float32)
    with torch.no_grad():
        model = HairGaussianModel.from_strands(moved, sh_degree=0, device="cpu", ref_strand_root=moved[:, 0])
    ply = os.path.join(root, "model", "point_cloud", "iteration_3", "point_cloud.ply")
    save_hair_ply(model, ply)
    return ply


def test_eval_cli_on_the_cpu_scores_a_saved_strand_model(tmp_path, capsys):
    import json
    import eval as eval_cli
    from data.eval_data import load_hair_eval_data_npz
    from loss.metrics import compute_metrics
    from utils.system import model_ply
    ply = _strand_capture(str(tmp_path / "capture"))
    out = tmp_path / "m.json"
    metrics, labels = eval_cli.main(["-s", str(tmp_path / "capture"), "-p", str(tmp_path / "capture" / "model"), "--device", "cpu",
                                     "--json", str(out)])
    text = capsys.readouterr().out
    assert "precision(b)" in text and "strand_consistency(b)" in text and labels[0] in text
    assert model_ply(str(tmp_path / "capture" / "model")) == ply
    # the same as scoring the model's own joints by hand
    pred = eval_cli.load_eval_data_from_gaussians(ply, device="cpu")
    want, _ = compute_metrics(pred, load_hair_eval_data_npz(str(tmp_path / "capture" / "hair_eval_data.npz")), bidirectional=True)
    assert want.keys() == metrics.keys() and all(np.array_equal(want[k], metrics[k]) for k in want)
    assert 0.5 < metrics["precision(b)"][-1] <= 1.0 and 0.5 < metrics["strand_consistency(b)"][-1] <= 1.0
    saved = json.loads(out.read_text())
    assert saved["thresholds"] == labels and saved["metrics"]["recall(b)"] == [float(x) for x in metrics["recall(b)"]]
    with pytest.raises(SystemExit):
        eval_cli.main(["-s", str(tmp_path), "-p", ply, "-pt", "neural_haircut"])
    # a metric without values (strand consistency of a Gaussian cloud, which has no strand ids) prints as "-"
    assert eval_cli.format_table({"recall(b)": np.array([0.5]), "strand_consistency(b)": np.array([])}, ["t"]).splitlines()[2].split() == \
        ["strand_consistency(b)", "-"]


def test_gpu_metrics_need_a_gpu_device():
    """No silent CPU fallback: a device the kernels cannot run on is an error, and so is a CUDA device on a host without a GPU
    (device=None and "cpu" select the CPU path)."""
    import torch
    import hgs_runtime as rt
    from loss.metrics import HairEvalData, compute_metrics
    d = HairEvalData(np.zeros((4, 3)), np.ones((4, 3)) / np.sqrt(3), np.arange(4))
    with pytest.raises(rt.HgsError):
        compute_metrics(d, d, device="meta")
    if not torch.cuda.is_available():
        with pytest.raises(rt.HgsError):
            compute_metrics(d, d, device="cuda")
    cpu, _ = compute_metrics(d, d, device="cpu")
    assert all(np.array_equal(v, compute_metrics(d, d)[0][k]) for k, v in cpu.items())
