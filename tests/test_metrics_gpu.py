"""Strand metrics on the GPU (csrc/hgs_metrics.hip through loss/metrics.py compute_metrics(device=...)): the same dict as the
CPU path, bit for bit, wherever the per-point matches agree; eval.py and train.py --eval_device on the device."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_PINS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_metrics_pins.npz"))
_NAMES = ("precision", "recall", "f1", "strand_consistency")


def _same(a, b):
    """Bitwise the same dict: keys, dtypes and bytes."""
    assert a.keys() == b.keys(), (a.keys(), b.keys())
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])


def _both(pred, gt, **kw):
    from loss.metrics import compute_metrics
    cpu = compute_metrics(pred, gt, **kw)
    gpu = compute_metrics(pred, gt, device="cuda", **kw)
    assert cpu[1] == gpu[1]
    _same(cpu[0], gpu[0])
    return gpu[0]


def _pins_case(ci):
    from loss.metrics import HairEvalData
    k = f"rand{ci}_"
    gt = HairEvalData(_PINS[k + "gt_points"], _PINS[k + "gt_dirs"], _PINS[k + "gt_strand"])
    pred = HairEvalData(_PINS[k + "pred_points"], _PINS[k + "pred_dirs"], _PINS[k + "pred_strand"])
    return pred, gt


@pytest.mark.parametrize("ci", [int(c) for c in _PINS["meta_cases"]])
@pytest.mark.parametrize("bidir", [False, True])
def test_pinned_cases_equal_the_cpu_path_and_the_reference(ci, bidir):
    pred, gt = _pins_case(ci)
    got = _both(pred, gt, bidirectional=bidir)
    want = _PINS[f"rand{ci}_metrics_b{int(bidir)}"]
    sfx = "(b)" if bidir else ""
    for j, nm in enumerate(_NAMES):
        assert np.allclose(got[nm + sfx], want[j], rtol=1e-12, atol=1e-15), (nm, bidir)


def test_boundary_masks_equal_ckdtree():
    from scipy.spatial import cKDTree
    from loss.metrics import HairEvalData, oriented_match
    from tests.test_metrics_contract_cpu import RADIUS, boundary_fixture
    a, b, inside = boundary_fixture()
    ones = np.tile([0.0, 0.0, 1.0], (len(a), 1))
    m = oriented_match(HairEvalData(a, ones), HairEvalData(b, ones), [RADIUS], [0.5])
    lists = cKDTree(b).query_ball_point(a, r=RADIUS)
    assert np.array_equal(m == 1, np.array([len(x) > 0 for x in lists])) and np.array_equal(m == 1, inside)


def _synthetic(n_strands, curly, seed):
    """GT as hair_eval_data.npz holds it (float64 unit directions) and a float32 prediction from other strands of the same head."""
    from synthetic import strand_polylines
    from loss.metrics import HairEvalData

    def side(pts, dtype):
        d = (pts[:, 1:] - pts[:, :-1]).astype(dtype)
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        ids = np.repeat(np.arange(pts.shape[0]), pts.shape[1] - 1)
        return HairEvalData(pts[:, :-1].reshape(-1, 3), d.reshape(-1, 3), ids)
    return (side(strand_polylines(n_strands, 100, seed=seed + 1, curly=curly), np.float32),
            side(strand_polylines(n_strands, 100, seed=seed, curly=curly), np.float64))


def _dot_margin_ok(a, b, dist_ths, angle_ths, bidir):
    """Precondition: no candidate within radius has its direction test within 1e-12 of cos_k (numpy's einsum sums the dot in
    an order that depends on the host's instruction set, so the last bit of a dot is not part of the contract)."""
    from scipy.spatial import cKDTree
    lists = cKDTree(b.points).query_ball_point(a.points, r=max(dist_ths))
    lens = np.fromiter((len(x) for x in lists), np.int64, len(lists))
    rows = np.repeat(np.arange(len(lists)), lens)
    cols = np.fromiter((j for x in lists for j in x), np.int64, int(lens.sum()))
    dot = np.einsum("ij,ij->i", np.asarray(a.directions, np.float64)[rows], np.asarray(b.directions, np.float64)[cols])
    if bidir:
        dot = np.abs(dot)
    cos = np.cos(np.deg2rad(np.asarray(angle_ths, np.float64)))
    return float(np.abs(dot[:, None] - cos[None, :]).min()) >= 1e-12


@pytest.mark.parametrize("n_strands,curly", [(2000, False), (10000, True)])
def test_large_strand_sets_equal_the_cpu_path(n_strands, curly):
    pred, gt = _synthetic(n_strands, curly, seed=7)
    assert len(gt.points) == 100 * n_strands
    d, a = (2e-3, 3e-3, 4e-3, 4e-3), (20, 30, 40, 90)
    assert _dot_margin_ok(pred, gt, d, a, True) and _dot_margin_ok(gt, pred, d, a, True)
    got = _both(pred, gt, bidirectional=True)
    assert got["recall(b)"][-1] > 0.1 and got["strand_consistency(b)"][-1] > 0.0


@pytest.mark.parametrize("capacity", [1, 4, 64])
def test_vote_table_overflow_recounts_on_the_host(capacity):
    from loss.metrics import compute_metrics
    pred, gt = _pins_case(int(_PINS["meta_cases"][0]))
    for bidir in (False, True):
        _same(compute_metrics(pred, gt, bidirectional=bidir)[0],
              compute_metrics(pred, gt, bidirectional=bidir, device="cuda", vote_capacity=capacity)[0])


def test_edge_cases_equal_the_cpu_path():
    from loss.metrics import HairEvalData
    rng = np.random.default_rng(3)
    n = 3000
    gt_p = rng.uniform(0, 0.05, (n, 3))
    gt_d = rng.normal(size=(n, 3)); gt_d /= np.linalg.norm(gt_d, axis=1, keepdims=True)
    pr_p = (gt_p + rng.normal(size=(n, 3)) * 2e-3).astype(np.float32)
    pr_d = (gt_d + rng.normal(size=(n, 3)) * 0.3).astype(np.float32)
    with np.errstate(invalid="ignore"):
        pr_d /= np.linalg.norm(pr_d, axis=1, keepdims=True)
    pr_d[::17] = np.nan                                         # zero-length segments: NaN directions never match
    gt_d[5::23] = np.nan
    ids_gt = rng.permutation(np.arange(n) // 7 * 13 + 1_000_000_007)   # unsorted, non-contiguous int64 strand ids
    ids_gt[::50] = rng.integers(2**40, 2**41, len(ids_gt[::50]))        # single-point strands
    ids_pr = rng.integers(-5, 5, n).astype(np.int64) * 3_000_000_000
    gt, pred = HairEvalData(gt_p, gt_d, ids_gt), HairEvalData(pr_p, pr_d, ids_pr)
    for bidir in (False, True):
        _both(pred, gt, bidirectional=bidir)                                          # (duplicate radii: 4 mm twice)
        _both(pred, gt, bidirectional=bidir, dist_ths=[3e-3], angle_ths=[30])         # K = 1
        radii = list(np.linspace(1e-3, 6e-3, 32))
        _both(pred, gt, bidirectional=bidir, dist_ths=radii, angle_ths=list(np.linspace(5, 90, 32)))   # K = 32
        _both(pred, gt, bidirectional=bidir, dist_ths=radii + [2e-3], angle_ths=list(np.linspace(5, 90, 32)) + [45])   # 2 passes
    empty = HairEvalData(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int64))
    with np.errstate(invalid="ignore", divide="ignore"):
        got = _both(empty, gt)
    assert np.isnan(got["precision"]).all() and got["f1"].dtype == np.int64
    from loss.metrics import compute_metrics
    for dev in (None, "cuda"):
        with pytest.raises(ZeroDivisionError), np.errstate(invalid="ignore", divide="ignore"):
            compute_metrics(gt, empty, device=dev)


def test_eval_cli_prints_the_same_table_on_both_devices(tmp_path, capsys):
    """eval.py on a strand model near the capture's strands and on a Stage-I cloud trained by train.py on a capture with
    hair_eval_data.npz: --device cuda and --device cpu print the same table."""
    import eval as eval_cli
    import train as train_cli
    from tests.test_dataset_io_cpu import _write_capture, _write_side_files
    from tests.test_metrics_contract_cpu import _strand_capture
    _strand_capture(str(tmp_path / "strands"))
    src, model = tmp_path / "capture", tmp_path / "out"
    _write_capture(src, n_views=3, W=64, H=48)
    _write_side_files(src)
    train_cli.main(["-s", str(src), "-m", str(model), "--iterations", "4", "--quiet"])
    for s, p in ((tmp_path / "strands", tmp_path / "strands" / "model"), (src, model)):
        tables = []
        for dev in ("cuda", "cpu"):
            capsys.readouterr()
            m, _ = eval_cli.main(["-s", str(s), "-p", str(p), "--device", dev])
            tables.append(capsys.readouterr().out.split("\n", 2)[2])      # (after the two "Loaded ..." lines)
        assert tables[0] == tables[1] and "precision(b)" in tables[0], tables


def test_train_eval_device_matches_the_cpu_evaluation_of_the_saved_model(tmp_path):
    import eval as eval_cli
    import train as train_cli
    from data.eval_data import load_hair_eval_data_npz
    from loss.metrics import compute_metrics
    from tests.test_dataset_io_cpu import _write_capture, _write_side_files
    from utils.system import model_ply
    src, model = tmp_path / "capture", tmp_path / "out"
    _write_capture(src, n_views=3, W=64, H=48)
    _write_side_files(src)
    scene = train_cli.main(["-s", str(src), "-m", str(model), "--iterations", "4", "--quiet", "--eval_device", "cuda"])
    pred = eval_cli.load_eval_data_from_gaussians(model_ply(str(model)), device="cuda")
    want, labels = compute_metrics(pred, load_hair_eval_data_npz(str(src / "hair_eval_data.npz")), bidirectional=True)   # (bidirectional_eval)
    assert scene.eval_thresholds == labels
    _same(want, scene.eval_metrics)
