"""Strand growth on the GPU (hgs_strand_grow_plan / hgs_strand_grow_fill behind HairTopologyMixin.growing): the device form
equals the host form (HGS_GROWTH=host) and the reference's own run (tests/golden/ref_growth_pins.npz) bit for bit, at 0, 1, 63,
64, 65 strands and at 4 10^5 segments; it is deterministic; training() grows strands at growth_interval with and without graph
replay; two view-parallel ranks grow alike; the train.py CLI runs Stage III with growth."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_growth_cpu as G

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _grow(build, monkeypatch, form, growth_length=0.002):
    """A fresh model from `build()` grown once by the device or the host form: (model, appended rows, counters, state before)."""
    monkeypatch.setenv("HGS_GROWTH", form)
    m = build()
    n0 = m.endpoint_pairs.shape[0]
    before = (m.endpoint_pairs.cpu().numpy().copy(), m._endpoints.shape[0], G.strand_tips(m))
    info = G.Info()
    m.growing(info, growth_length=growth_length)
    return m, G.grown_rows(m, n0), info.densification_info, before


def _assert_rows_equal(a, b, what):
    for name, x, y in zip(("pairs", "endpoints") + G.GROUPS[1:], a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name)


def _strand_model(S, n_seg=8, seed=0, sh_degree=3, k_avg=3, num_points_strand=80):
    """S random strands of n_seg segments on the GPU with distinct attributes, some tips collapsed, some strands at the limit."""
    from arguments import OptimizationParams
    from scene.hair_gaussian_model import HairGaussianModel
    from synthetic import strand_polylines
    pts = strand_polylines(max(S, 1), n_seg, seed=seed).astype(np.float32)
    rng = np.random.default_rng(seed)
    pts[1::7, -1] = pts[1::7, -2]                       # last segment collapsed
    pts[2::7, -4:] = pts[2::7, -5:-4]                   # last four collapsed
    m = HairGaussianModel.from_strands(pts, device="cuda", sh_degree=sh_degree)
    opt = OptimizationParams()
    opt.num_points_strand, opt.growth_averaging_points = num_points_strand, k_avg
    m.training_setup(opt)
    P = m.endpoint_pairs.shape[0]
    with torch.no_grad():
        for t in (m._features_dc, m._features_rest, m._opacity, m._width):
            t.add_(torch.from_numpy(rng.normal(size=tuple(t.shape)).astype(np.float32)).cuda() * 0.1)
        m._mask.copy_(torch.from_numpy(rng.uniform(0.5, 3.0, size=(P, 1)).astype(np.float32)).cuda())
        if S == 0:
            m._mask.fill_(-5.0)                         # every segment in the background: no strand
    m.compute_strands_info()
    assert m.strands_info.n_strands == S
    return m


@pytest.mark.parametrize("S", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("k_avg,growth_length", [(3, 0.002), (10, None), (32, 0.004)])
def test_device_growth_equals_host(monkeypatch, S, k_avg, growth_length):
    build = lambda: _strand_model(S, n_seg=12, seed=S, k_avg=k_avg)
    md, dev, info_d, before = _grow(build, monkeypatch, "device", growth_length)
    _, host, info_h, _ = _grow(build, monkeypatch, "host", growth_length)
    assert info_d == info_h
    _assert_rows_equal(dev, host, S)
    assert (info_d["grow"] > 0) == (S > 0)
    if info_d["grow"]:
        G.assert_consistent_after_growth(md, before, info_d["grow"])


def test_device_growth_equals_the_reference_run(monkeypatch):
    pins = np.load(os.path.join(ROOT, "tests", "golden", "ref_growth_pins.npz"))
    monkeypatch.setenv("HGS_GROWTH", "device")
    for case in G.pin_cases(pins):
        m = G.model_for_pin(pins, case, device="cuda")
        n0 = m.endpoint_pairs.shape[0]
        info = G.Info()
        m.growing(info, growth_length=G.growth_length_of(pins, case))
        want = G.pinned_rows(pins, case)
        assert info.densification_info["grow"] == want[0].shape[0], case
        for name, a, b in zip(("pairs", "endpoints") + G.GROUPS[1:], G.grown_rows(m, n0), want):
            assert a.size == b.size and a.reshape(-1).tobytes() == b.astype(a.dtype).reshape(-1).tobytes(), (case, name)


def test_device_growth_with_background_and_shared_tips(monkeypatch):
    for seed in range(4):
        build = lambda: G.growth_model(seed, background=True, device="cuda", k_avg=5)
        want, counter, shared = G.restated_growth(build(), None)
        _, dev, info, _ = _grow(build, monkeypatch, "device", None)
        assert info == {"grow": counter, "grow_skipped_shared_tip": shared}
        _assert_rows_equal(dev, want, seed)


def test_device_growth_at_a_merged_model_size(monkeypatch):
    """4 10^5 segments (20 000 strands): device == host, bit for bit; a repeated event gives the same bits."""
    build = lambda: _strand_model(20000, n_seg=20, seed=5, k_avg=5)
    md, dev, info_d, before = _grow(build, monkeypatch, "device", None)
    assert before[0].shape[0] >= 4 * 10 ** 5
    _, dev2, info_d2, _ = _grow(build, monkeypatch, "device", None)
    _, host, info_h, _ = _grow(build, monkeypatch, "host", None)
    assert info_d == info_d2 == info_h and info_d["grow"] > 15000
    _assert_rows_equal(dev, dev2, "repeat")
    _assert_rows_equal(dev, host, "host")
    G.assert_consistent_after_growth(md, before, info_d["grow"])


def _assert_model_sane(model):
    P, E = model.endpoint_pairs.shape[0], model._endpoints.shape[0]
    assert int(model.endpoint_pairs.max()) == E - 1
    assert int(torch.bincount(model.endpoint_pairs.reshape(-1)).max()) <= 2          # still chains
    for g in model.optimizer.param_groups:
        p = g["params"][0]
        assert torch.isfinite(p).all() and p.shape[0] == (E if g["name"] == "endpoints" else P)
        st = model.optimizer.state.get(p, {})
        for mom in ("exp_avg", "exp_avg_sq"):
            assert mom not in st or st[mom].shape == p.shape
    for t in (model.xyz_gradient_accum, model.denom, model.max_radii2D):
        assert t.shape[0] == P


@pytest.mark.parametrize("use_graph", [False, True])
def test_training_grows_strands_at_the_growth_interval(use_graph):
    from arguments import OptimizationParams
    from synthetic import build_workload
    from train import training
    from utils.general import safe_state
    safe_state(True)
    model, cams, extent = build_workload("tiny", device="cuda", with_targets=True)
    opt = OptimizationParams()
    opt.growth_interval = 6
    model.training_setup(opt)
    P0 = model.get_xyz.shape[0]
    events = []
    ema = training(model, cams, opt, iterations=14, extent=extent, use_graph=use_graph, event_log=events)
    assert torch.isfinite(ema)
    grows = [e for e in events if "grow" in e]
    assert [e["iteration"] for e in grows] == [6, 12] and all(e["grow"] > 0 for e in grows), events
    assert model.get_xyz.shape[0] == P0 + sum(e["grow"] for e in grows)
    _assert_model_sane(model)


def test_two_ranks_grow_alike():
    from tests.gpu_util import free_port
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(ROOT, "tests", "_vp_growth_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), worker]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "VP_GROWTH_OK" in out.stdout


def test_train_cli_stage_three_grows(tmp_path):
    from tests.test_dataset_io_cpu import _write_capture, _write_side_files
    import merge as merge_cli
    import train as train_cli
    from scene.hair_gaussian_model import HairGaussianModel
    src, model = tmp_path / "capture", tmp_path / "out"
    _write_capture(src, n_views=4, W=96, H=64)
    _write_side_files(src)
    train_cli.main(["-s", str(src), "-m", str(model), "--iterations", "10", "--save_frequency", "10", "--quiet"])
    merge_cli.main(["-s", str(src), "-m", str(model), "--iterations", "3"])
    s3 = train_cli.main(["-s", str(src), "-m", str(model), "--iterations", "8", "--save_frequency", "8", "--quiet",
                         "--growth_interval", "4"])
    g = s3.gaussians
    assert isinstance(g, HairGaussianModel) and g.strands_info is not None
    _assert_model_sane(g)
